"""numpy restatement of the 512 x 320 try-on set's per-pair preparation (reference training/dataset.py,
``UvitonDatasetFull_512_test``: ``_load_raw_image`` :1605-1695, ``get_hand_mask`` / ``get_palm`` :1779-1827,
``draw_pose_from_cords`` :1831-1864, ``get_crop`` :1879-1965, ``normalize_full`` / ``normalize_upper`` / ``normalize_lower``
:1967-2193, ``__getitem__`` :2196-2214) and of test_512.py's tensor expressions (:115-131) and panels (:144-188), one pair at a
time.  The region entries of csrc/tryon_pairs.hip and training/tryon_regions.py are held to it bit for bit
(tests/test_tryon_512_gpu.py).

Built from the primitives of tests/tryon_ref.py (rleFrPoly fill, box dilation, palm rule), tests/tryon_pairs_ref.py (erode)
and oracle/ref_patches.py (warpPerspective, getPerspectiveTransform, get_crop's quadrilaterals with x_pad = 0), with own
variants where those fix a size or a thickness: the thickness-5 line, the radius-5 disc, the 512 square and its boxes 35 / 20,
get_crop without the shin fall-back.  Parity with OpenCV, pycocotools and skimage themselves is UNPINNED, as for the 256 sets;
``thick_line`` for thickness 5 is this project's restatement of cv2's thick line (a polygon of half-width t / 2 with round
caps): every pixel centre within t / 2 of the segment."""
import numpy as np

import tryon_pairs_ref as PR
import tryon_ref as R
from oracle import ref_patches as RP

SIDE = 512
CANVAS = (512, 320)
PALM_BOXES = (35, 20)
LOWER_PARTS = (0, 6, 7, 8, 9)
REGIONS = ('fullbody', 'upperbody', 'lowerbody')


def thick_line(img, p, q, color, thickness):
    """cv2.line(img, p, q, color, thickness) restated: pixels (x, y) within distance thickness / 2 of the segment p -> q
    (integer points), in integers: 4 d^2 <= t^2 at the ends, 4 cross^2 <= t^2 len2 along it."""
    h, w = img.shape[:2]
    ys, xs = np.mgrid[0:h, 0:w].astype(np.int64)
    x0, y0 = p
    x1, y1 = q
    t2 = thickness * thickness
    dx, dy = x1 - x0, y1 - y0
    ux, uy = xs - x0, ys - y0
    len2 = dx * dx + dy * dy
    t = ux * dx + uy * dy
    near0 = 4 * (ux * ux + uy * uy) <= t2
    near1 = 4 * ((xs - x1) ** 2 + (ys - y1) ** 2) <= t2
    if len2 == 0:
        hit = near0
    else:
        hit = np.where(t <= 0, near0, np.where(t >= len2, near1, 4 * (ux * dy - uy * dx) ** 2 <= t2 * len2))
    img[hit] = color


def disc(shape, r, c, radius):
    """skimage.draw.circle(r, c, radius, shape) as a boolean image: _ellipse_in_shape with rotation 0, in float64."""
    rr, cc = np.mgrid[0:shape[0], 0:shape[1]]
    return ((rr - r) / radius) ** 2 + ((cc - c) / radius) ** 2 < 1


def draw_pose_from_cords(pose_joints, img_size=CANVAS, thickness=5, radius=5):
    """dataset.py:1831-1864 (no affine): limbs with the restated thick line, then the joint discs."""
    colors = np.zeros(tuple(img_size) + (3,), dtype=np.uint8)
    for i, p in enumerate(R.LIMBSEQ):
        f, t = p[0] - 1, p[1] - 1
        if pose_joints[f][2] < 0.1 or pose_joints[t][2] < 0.1:
            continue
        pf = pose_joints[f][0], pose_joints[f][1]
        pt = pose_joints[t][0], pose_joints[t][1]
        fx, fy = int(pf[1]), int(pf[0])
        tx, ty = int(pt[1]), int(pt[0])
        thick_line(colors, (fy, fx), (ty, tx), R.KPTCOLORS[i], thickness)
    for i, joint in enumerate(pose_joints):
        if pose_joints[i][2] < 0.1:
            continue
        x, y = int(joint[1]), int(joint[0])
        colors[disc(img_size, x, y, radius)] = R.KPTCOLORS[i]
    return colors


def hand_masks(arm, side=SIDE, boxes=PALM_BOXES):
    """get_hand_mask (:1779-1799) for shoulder, elbow, wrist rows of already shifted key points."""
    up, bottom = np.ones((side, side), np.float32), np.ones((side, side), np.float32)
    (s_x, s_y, s_c), (e_x, e_y, e_c), (w_x, w_y, w_c) = arm
    if s_c > 0.1 and e_c > 0.1:
        up = (R.dilate(R.get_rectangle_mask(s_x, s_y, e_x, e_y, side, side), boxes[0]) > 0).astype(np.float32)
    if e_c > 0.1 and w_c > 0.1:
        bottom = (R.dilate(R.get_rectangle_mask(e_x, e_y, w_x, w_y, side, side), boxes[1]) > 0).astype(np.float32)
    return up, bottom


def palm_mask(shifted_kp, parsing_padded, boxes=PALM_BOXES):
    """get_palm (:1809-1827) on key points already shifted by the padding; parsing_padded [S, S]."""
    palms = []
    for rows, label in (([5, 6, 7], 14), ([2, 3, 4], 15)):
        up, bottom = hand_masks(shifted_kp[rows], parsing_padded.shape[0], boxes)
        palms.append(R.get_palm_mask((parsing_padded == label).astype(np.float32), up, bottom))
    return ((palms[0] + palms[1]) > 0).astype(np.uint8)


def crop_matrices(shifted_kp, bpart, o_w, o_h, box_factor=2):
    """get_crop (:1879-1965): (M, M_inv) or (None, None).  The quadrilateral is oracle/ref_patches.part_quadrilateral's with
    x_pad = 0: the thigh falls back to a segment from the hip to row o_h - 1, the shin has no fall-back (:1893-1900)."""
    quad = RP.part_quadrilateral(shifted_kp, bpart, o_h, x_pad=0)
    if quad is None:
        return None, None
    w, h = o_w // 2 ** box_factor, o_h // 2 ** box_factor
    corners = np.float32([[0.0, 0.0], [0.0, 1.0], [1.0, 1.0], [1.0, 0.0]]) * np.float32([[w, h]])
    return RP.get_perspective_transform(quad, corners), RP.get_perspective_transform(corners, quad)


def region_sources(region):
    """(upper garment from the donor, lower garment from the donor) of :1679-1690."""
    return dict(fullbody=(True, True), upperbody=(True, False), lowerbody=(False, True))[region]


def normalize_region(region, upper_img, lower_img, upper_mask, lower_mask, clothes_kp, person_kp, box_factor=2):
    """normalize_full / normalize_upper / normalize_lower (:1967-2193), which differ only in whose M warps each garment forward:
    the donor's (clothes_M) or the person's (person_M), as the garment's source.  Every part goes back with the person's M_inv
    and a 5 x 5 eroded mask.  -> (norm_img [h,w,30], norm_img_lower [h,w,15], mask patches [h,w,30], [h,w,15], denorm_upper,
    denorm_lower [H,W,3])."""
    upper_donor, lower_donor = region_sources(region)
    o_h, o_w = upper_img.shape[:2]
    h, w = o_h // 2 ** box_factor, o_w // 2 ** box_factor
    imgs, imgs_l, masks, masks_l = [], [], [], []
    den_u, den_l = np.zeros_like(upper_img), np.zeros_like(upper_img)

    def back(den, p_img, p_mask, m_inv):
        patch = RP.warp_perspective(p_img, m_inv, (o_w, o_h), RP.BORDER_CONSTANT)
        mask = RP.warp_perspective(p_mask, m_inv, (o_w, o_h), RP.BORDER_CONSTANT)[..., 0:1]
        hit = (PR.erode(mask, 5) == 255).astype(np.uint8)
        return patch * hit + den * (1 - hit)

    for ii, bpart in enumerate(RP.PARTS):
        blank = np.zeros((h, w, 3), np.uint8)
        p_img, p_mask, p_img_l, p_mask_l = blank, blank, blank, blank
        clothes_m, _ = crop_matrices(clothes_kp, bpart, o_w, o_h, box_factor)
        person_m, person_m_inv = crop_matrices(person_kp, bpart, o_w, o_h, box_factor)
        m_up = clothes_m if upper_donor else person_m
        m_lo = clothes_m if lower_donor else person_m
        if m_up is not None:
            p_img = RP.warp_perspective(upper_img, m_up, (w, h), RP.BORDER_REPLICATE)
            p_mask = RP.warp_perspective(upper_mask, m_up, (w, h), RP.BORDER_REPLICATE)
        if person_m_inv is not None:
            den_u = back(den_u, p_img, p_mask, person_m_inv)
        imgs.append(p_img)
        masks.append(p_mask)
        if ii == 0 or ii >= 6:
            if m_lo is not None:
                p_img_l = RP.warp_perspective(lower_img, m_lo, (w, h), RP.BORDER_REPLICATE)
                p_mask_l = RP.warp_perspective(lower_mask, m_lo, (w, h), RP.BORDER_REPLICATE)
            if person_m_inv is not None:
                den_l = back(den_l, p_img_l, p_mask_l, person_m_inv)
            imgs_l.append(p_img_l)
            masks_l.append(p_mask_l)
    cat = lambda xs: np.concatenate(xs, axis=2)
    return cat(imgs), cat(imgs_l), cat(masks), cat(masks_l), den_u, den_l


def person_stages(image_unpadded, parsing_unpadded, kp):
    """The padded image, stick figure, parsing [S,S,1] and the float64-shifted key points of one person (:1608-1629)."""
    h, w = image_unpadded.shape[:2]
    lp, rp = (h - w) // 2, h - w - (h - w) // 2
    image = np.pad(image_unpadded, ((0, 0), (lp, rp), (0, 0)), 'constant', constant_values=(255, 255))
    pose = np.pad(draw_pose_from_cords(kp, (h, w)), ((0, 0), (lp, rp), (0, 0)), 'constant', constant_values=(0, 0))
    parsing = np.pad(parsing_unpadded[..., None], ((0, 0), (lp, rp), (0, 0)), 'constant', constant_values=(0, 0))
    shifted = np.array(kp, np.float64)
    shifted[:, 0] += lp
    return image, pose, parsing, shifted


def garments(image, parsing):
    """(upper image, lower image, upper mask rgb, lower mask rgb) of one padded person (:1637-1647, :1667-1677)."""
    upper = sum((parsing == v).astype(np.uint8) for v in (5, 6, 7))
    lower = sum((parsing == v).astype(np.uint8) for v in (9, 12))
    return upper * image, lower * image, np.concatenate([upper] * 3, axis=2) * 255, np.concatenate([lower] * 3, axis=2) * 255


def label_stages(raw, region):
    """_load_raw_image (:1605-1677) up to the call of normalize_*: the uint8 stages, the garments already picked by the region."""
    image, pose, parsing, kp = person_stages(raw['image'], raw['parsing'], raw['keypoints'])
    shoes = sum((parsing == v).astype(np.uint8) for v in (18, 19))
    head = sum((parsing == v).astype(np.uint8) for v in (1, 2, 4, 13))
    palm = palm_mask(kp, parsing[..., 0])[..., None]
    retain_mask = shoes + palm + head
    clothes, _, c_parsing, c_kp = person_stages(raw['clothes_image'], raw['clothes_parsing'], raw['clothes_keypoints'])
    person_g, clothes_g = garments(image, parsing), garments(clothes, c_parsing)
    upper_donor, lower_donor = region_sources(region)
    up, lo = (clothes_g if upper_donor else person_g), (clothes_g if lower_donor else person_g)
    return dict(image=image, clothes=clothes, stick=pose, palm=palm[..., 0], retain_mask=retain_mask, retain_img=retain_mask * image,
                upper_img=up[0], upper_mask=up[2], lower_img=lo[1], lower_mask=lo[3], kp=kp, clothes_kp=c_kp)


def load_pair(raw, region):
    """_load_raw_image (:1605-1695) of one raw pair (a dict of UvitonDatasetFull_512_test): a dict of the uint8 stages."""
    s = label_stages(raw, region)
    norm_img, norm_lower, mask_patches, mask_patches_l, den_u, den_l = normalize_region(
        region, s['upper_img'], s['lower_img'], s['upper_mask'], s['lower_mask'], s['clothes_kp'], s['kp'])
    s.update(patches=norm_img, patches_lower=norm_lower, mask_patches=mask_patches, mask_patches_lower=mask_patches_l, denorm_upper=den_u,
             denorm_lower=den_l)
    return s


def getitem(stages):
    """__getitem__ (:2196-2214): (image, clothes, pose, norm_img, norm_img_lower, denorm_upper, denorm_lower, denorm_upper_mask,
    denorm_lower_mask, retain_mask) uint8 CHW."""
    chw = lambda a: a.transpose(2, 0, 1).copy()
    du, dl = chw(stages['denorm_upper']), chw(stages['denorm_lower'])
    masks = [(np.sum(d, axis=0, keepdims=True) > 0).astype(np.uint8) for d in (du, dl)]
    return (chw(stages['image']), chw(stages['clothes']), chw(stages['stick']), chw(stages['patches']), chw(stages['patches_lower']), du, dl,
            masks[0], masks[1], chw(stages['retain_mask']))


def generator_inputs(items, device):
    """test_512.py:115-131 on a batch of getitem tuples, with torch on ``device`` as the reference does it: the nine tensors of
    training.tryon_regions.TryOnRegionBatch.KEYS."""
    import torch
    image, clothes, pose, norm_img, norm_img_lower, du, dl, um, lm, retain_mask = (torch.from_numpy(np.stack([it[k] for it in items]))
                                                                                   for k in range(10))
    image_tensor = image.to(device).to(torch.float32) / 127.5 - 1
    clothes_tensor = clothes.to(device).to(torch.float32) / 127.5 - 1
    pose_tensor = pose.to(device).to(torch.float32) / 127.5 - 1
    norm_img_tensor = norm_img.to(device).to(torch.float32) / 127.5 - 1
    norm_img_lower_tensor = norm_img_lower.to(device).to(torch.float32) / 127.5 - 1
    parts_tensor = torch.cat([norm_img_tensor, norm_img_lower_tensor], dim=1)
    denorm_upper_clothes_tensor = du.to(device).to(torch.float32) / 127.5 - 1
    denorm_upper_mask_tensor = um.to(device).to(torch.float32)
    denorm_lower_clothes_tensor = dl.to(device).to(torch.float32) / 127.5 - 1
    denorm_lower_mask_tensor = lm.to(device).to(torch.float32)
    retain_mask_tensor = retain_mask.to(device)
    retain_tensor = image_tensor * retain_mask_tensor - (1 - retain_mask_tensor)
    pose_tensor = torch.cat([pose_tensor, retain_tensor], dim=1)
    return dict(image=image_tensor, clothes=clothes_tensor, retain=retain_tensor, pose=pose_tensor, style_input=parts_tensor,
                denorm_upper_input=denorm_upper_clothes_tensor, denorm_lower_input=denorm_lower_clothes_tensor,
                denorm_upper_mask=denorm_upper_mask_tensor, denorm_lower_mask=denorm_lower_mask_tensor)


def panel(img_chw, clip):
    """test_512.py:145-159 for one fp32 [3, H, W] numpy image: (x + 1.0) * 127.5 in float32, [clipped,] truncated, BGR for
    cv2.imwrite -- returned as the RGB picture that file holds."""
    img = (img_chw.transpose(1, 2, 0) + 1.0) * 127.5
    if clip:
        img = np.clip(img, 0, 255)
    return img.astype(np.uint8)[..., [2, 1, 0]][..., ::-1]


def result_image(clothes_chw, image_chw, gen_chw):
    """test_512.py:180: clothes | person | generated, [H, 3W, 3] RGB."""
    return np.concatenate([panel(clothes_chw, False), panel(image_chw, False), panel(gen_chw, True)], axis=1)
