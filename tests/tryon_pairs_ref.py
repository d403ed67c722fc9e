"""numpy restatement of the try-on TEST set's per-pair preparation (reference training/dataset.py: ``_load_raw_image``
:1085-1153, ``get_hand_mask`` / ``get_palm`` :1240-1282, ``get_crop`` :1341-1428, ``normalize`` :1430-1500, ``__getitem__``
:1502-1525) and of test.py's conversions (:104-117, :133-137), one pair at a time.  The kernels of csrc/tryon_pairs.hip and
training/tryon_pairs.py are held to it bit for bit (tests/test_tryon_pairs_gpu.py).

Built from the primitives of tests/tryon_ref.py (stick figure, rleFrPoly fill, box dilation, palm rule) and of
oracle/ref_patches.py (warpPerspective, getPerspectiveTransform, get_crop's quadrilaterals with x_pad = 0), plus a brute-force
``cv2.erode``.  Parity with OpenCV, pycocotools and skimage themselves is UNPINNED, as for the training set."""
import numpy as np

import tryon_ref as R
from oracle import ref_patches as RP

UPPER_PARTS = 6


def erode(img, k):
    """cv2.erode(img, np.ones((k, k))) by brute force, per channel: the minimum over offsets -(k // 2) .. k - 1 - k // 2, pixels
    outside the image left out (cv2's default border for erosion)."""
    h, w = img.shape[:2]
    a = k // 2
    pad = np.full((h + k - 1, w + k - 1) + img.shape[2:], 255, img.dtype)
    pad[a:a + h, a:a + w] = img
    out = np.full_like(img, 255)
    for dy in range(k):
        for dx in range(k):
            out = np.minimum(out, pad[dy:dy + h, dx:dx + w])
    return out


def hand_masks(arm, forearm_box=15):
    """get_hand_mask (:1240-1256) for shoulder, elbow, wrist rows of already shifted key points: the 25 x 25 box of the upper
    arm and the forearm_box one of the forearm (15 at test time; training: 16)."""
    up, bottom = np.ones((256, 256), np.float32), np.ones((256, 256), np.float32)
    (s_x, s_y, s_c), (e_x, e_y, e_c), (w_x, w_y, w_c) = arm
    if s_c > 0.1 and e_c > 0.1:
        up = (R.dilate(R.get_rectangle_mask(s_x, s_y, e_x, e_y, 256, 256), 25) > 0).astype(np.float32)
    if e_c > 0.1 and w_c > 0.1:
        bottom = (R.dilate(R.get_rectangle_mask(e_x, e_y, w_x, w_y, 256, 256), forearm_box) > 0).astype(np.float32)
    return up, bottom


def palm_mask(shifted_kp, parsing_padded, forearm_box=15):
    """get_palm (:1266-1282) on key points already shifted by the padding; parsing_padded [256, 256]."""
    palms = []
    for rows, label in (([5, 6, 7], 14), ([2, 3, 4], 15)):
        up, bottom = hand_masks(shifted_kp[rows], forearm_box)
        palms.append(R.get_palm_mask((parsing_padded == label).astype(np.float32), up, bottom))
    return ((palms[0] + palms[1]) > 0).astype(np.uint8)


def crop_matrices(shifted_kp, bpart, o_w, o_h, box_factor=2):
    """get_crop (:1341-1428): (M, M_inv) or (None, None).  The quadrilateral is oracle/ref_patches.part_quadrilateral's with
    x_pad = 0 (the key points come shifted in float64), plus the test set's own fall-back of a shin without its ankle: a
    segment from the knee straight down to the last row, as the thigh's."""
    quad = RP.part_quadrilateral(shifted_kp, bpart, o_h, x_pad=0)
    knee = RP.ORDER.index(bpart[0])
    if quad is None and bpart[0] in ('lknee', 'rknee') and shifted_kp[knee, 2] >= 0.1:
        top = np.float32(shifted_kp[[knee]][:, :2])[0]
        bottom = np.float32([top[0], o_h - 1])
        seg = bottom - top
        half = np.array([-seg[1], seg[0]]) * 0.25
        quad = np.float32([top + half, top - half, bottom - half, bottom + half])
    if quad is None:
        return None, None
    w, h = o_w // 2 ** box_factor, o_h // 2 ** box_factor
    corners = np.float32([[0.0, 0.0], [0.0, 1.0], [1.0, 1.0], [1.0, 0.0]]) * np.float32([[w, h]])
    return RP.get_perspective_transform(quad, corners), RP.get_perspective_transform(corners, quad)


def normalize_pair(upper_img, lower_img, upper_mask, lower_mask, upper_pose, lower_pose, upper_kp, lower_kp, box_factor=2):
    """normalize (:1430-1500): parts 0..5 from the donor (upper_*) with its matrices, 6..9 from the person (lower_*); every
    part back with the person's M_inv, the masks of parts 0..5 eroded 5 x 5 before the == 255 test.
    -> (patches [h,w,30], stick patches [h,w,30], mask patches [h,w,30], denorm_upper, denorm_lower [H,W,3])."""
    o_h, o_w = upper_img.shape[:2]
    h, w = o_h // 2 ** box_factor, o_w // 2 ** box_factor
    imgs, sticks, masks = [], [], []
    den_u, den_l = np.zeros_like(upper_img), np.zeros_like(upper_img)
    for ii, bpart in enumerate(RP.PARTS):
        blank = np.zeros((h, w, 3), np.uint8)
        p_img, p_stick, p_mask = blank, blank, blank
        m_up, _ = crop_matrices(upper_kp, bpart, o_w, o_h, box_factor)
        m_lo, m_lo_inv = crop_matrices(lower_kp, bpart, o_w, o_h, box_factor)
        source = (m_up, upper_img, upper_pose, upper_mask) if ii < UPPER_PARTS else (m_lo, lower_img, lower_pose, lower_mask)
        if source[0] is not None:
            p_img, p_stick, p_mask = (RP.warp_perspective(s, source[0], (w, h), RP.BORDER_REPLICATE) for s in source[1:])
        if m_lo_inv is not None:
            back = RP.warp_perspective(p_img, m_lo_inv, (o_w, o_h), RP.BORDER_CONSTANT)
            back_mask = RP.warp_perspective(p_mask, m_lo_inv, (o_w, o_h), RP.BORDER_CONSTANT)
            if ii < UPPER_PARTS:
                back_mask = erode(back_mask, 5)
            hit = (back_mask[..., 0:1] == 255).astype(np.uint8)
            if ii < UPPER_PARTS:
                den_u = back * hit + den_u * (1 - hit)
            else:
                den_l = back * hit + den_l * (1 - hit)
        imgs.append(p_img)
        sticks.append(p_stick)
        masks.append(p_mask)
    cat = lambda xs: np.concatenate(xs, axis=2)
    return cat(imgs), cat(sticks), cat(masks), den_u, den_l


def person_stages(image_unpadded, parsing_unpadded, kp):
    """The padded image, stick figure, parsing [H,H,1] and the float64-shifted key points of one person (:1085-1104)."""
    h, w = image_unpadded.shape[:2]
    lp, rp = (h - w) // 2, h - w - (h - w) // 2
    image = np.pad(image_unpadded, ((0, 0), (lp, rp), (0, 0)), 'constant', constant_values=(255, 255))
    pose = np.pad(R.draw_pose_from_cords(kp, (h, w)), ((0, 0), (lp, rp), (0, 0)), 'constant', constant_values=(0, 0))
    parsing = np.pad(parsing_unpadded[..., None], ((0, 0), (lp, rp), (0, 0)), 'constant', constant_values=(0, 0))
    shifted = np.array(kp, np.float64)
    shifted[:, 0] += lp
    return image, pose, parsing, shifted


def load_pair(raw):
    """_load_raw_image (:1085-1153) of one raw pair (a dict of UvitonDatasetV19_test): a dict of the uint8 stages."""
    image, pose, parsing, kp = person_stages(raw['image'], raw['parsing'], raw['keypoints'])
    palm = palm_mask(kp, parsing[..., 0])[..., None]
    head = sum((parsing == v).astype(np.uint8) for v in (1, 4, 2, 13))
    shoes = sum((parsing == v).astype(np.uint8) for v in (18, 19))
    lower = sum((parsing == v).astype(np.uint8) for v in (9, 12, 6))
    lower_img = lower * image
    retain_img = image * (palm + head + shoes)
    clothes, c_pose, c_parsing, c_kp = person_stages(raw['clothes_image'], raw['clothes_parsing'], raw['clothes_keypoints'])
    upper = sum((c_parsing == v).astype(np.uint8) for v in (5, 6, 7))
    upper_img = upper * clothes
    upper_mask = np.concatenate([upper] * 3, axis=2) * 255
    lower_mask = np.concatenate([lower] * 3, axis=2) * 255
    patches, stick_patches, mask_patches, den_u, den_l = normalize_pair(upper_img, lower_img, upper_mask, lower_mask, c_pose, pose, c_kp, kp)
    return dict(palm=palm[..., 0], retain_img=retain_img, stick=pose, clothes_stick=c_pose, lower_img=lower_img, lower_mask=lower_mask,
                upper_img=upper_img, upper_mask=upper_mask, patches=patches, stick_patches=stick_patches, mask_patches=mask_patches,
                denorm_upper=den_u, denorm_lower=den_l)


def getitem(stages):
    """__getitem__ (:1502-1525): (image, pose, norm_img [60,h,w], denorm_upper, denorm_lower, upper_mask, lower_mask) uint8 CHW."""
    chw = lambda a: a.transpose(2, 0, 1)
    norm_img = np.concatenate((chw(stages['patches']), chw(stages['stick_patches'])), axis=0)
    du, dl = chw(stages['denorm_upper']), chw(stages['denorm_lower'])
    masks = [(np.sum(d, axis=0, keepdims=True) > 0).astype(np.uint8) for d in (du, dl)]
    return chw(stages['retain_img']), chw(stages['stick']), norm_img, du, dl, masks[0], masks[1]


def generator_inputs(items, device):
    """test.py:104-117 on a batch of getitem tuples, with torch on ``device`` as the reference does it: the seven tensors of
    training.tryon_pairs.TryOnPairBatch.KEYS."""
    import torch
    cols = [torch.from_numpy(np.stack([it[k] for it in items])) for k in range(7)]
    image, pose, norm_img, du, dl, um, lm = cols
    unit = lambda t: t.to(device).to(torch.float32) / 127.5 - 1
    image_t = unit(image)
    return dict(retain=image_t, pose=torch.cat([unit(pose), image_t], dim=1), style_input=unit(norm_img), denorm_upper_input=unit(du),
                denorm_lower_input=unit(dl), denorm_upper_mask=um.to(device).to(torch.float32), denorm_lower_mask=lm.to(device).to(torch.float32))


def image_to_u8(gen_img_chw, c0=32, c1=224):
    """test.py:133-137 for one fp32 [3, H, Wt] numpy image: (x + 1.0) * 127.5 in float32, columns c0:c1, clipped and truncated.
    cv2.imwrite of the BGR-swapped array stores the RGB image: this returns that RGB image [H, c1 - c0, 3]."""
    img = (gen_img_chw.transpose(1, 2, 0) + 1.0) * 127.5
    img = img[:, c0:c1, [2, 1, 0]]
    img = np.clip(img, 0, 255).astype(np.uint8)
    return img[..., ::-1]
