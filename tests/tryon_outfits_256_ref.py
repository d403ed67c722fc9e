"""numpy restatement of a 256 x 192 OUTFIT (this project's own rules, include/pasta_hip.h): a person P in the upper garment of U
and the lower garment of L, one outfit at a time.  Only glue is new here: every step is a primitive of tests/tryon_pairs_ref.py
(``person_stages``, ``palm_mask``, ``crop_matrices``, the brute-force ``erode``) or of oracle/ref_patches.py
(``warp_perspective``), put together as ``tryon_pairs_ref.load_pair`` / ``normalize_pair`` put them together for a pair, with
three people where those have two and the lower garment's erosion where L is not P.  ``tryon_pairs_ref.getitem`` and
``generator_inputs`` take the stages unchanged."""
import numpy as np

import tryon_pairs_ref as PR
from oracle import ref_patches as RP

UPPER_PARTS = PR.UPPER_PARTS
ERODE = 5                   # cv2.erode(..., np.ones((5, 5))): parts 0..5 always, parts 6..9 where the lower garment is somebody else's


def normalize_outfit(upper_img, lower_img, upper_mask, lower_mask, upper_pose, lower_pose, upper_kp, lower_kp, person_kp, own_lower,
                     box_factor=2):
    """``tryon_pairs_ref.normalize_pair`` with the person's key points apart from the lower garment's owner's: parts 0..5 from U
    with U's matrices, parts 6..9 from L with L's, every part back with P's M_inv; the masks of parts 0..5 eroded, those of parts
    6..9 eroded unless ``own_lower``.  -> (patches, stick patches, mask patches [h,w,30], denorm_upper, denorm_lower [H,W,3],
    the lower composite without the erosion, the lower composite with it or None where ``own_lower``: it is not formed there)."""
    o_h, o_w = upper_img.shape[:2]
    h, w = o_h // 2 ** box_factor, o_w // 2 ** box_factor
    imgs, sticks, masks = [], [], []
    den_u, den_l_plain = np.zeros_like(upper_img), np.zeros_like(upper_img)
    den_l_eroded = None if own_lower else np.zeros_like(upper_img)

    def put(den, back, back_mask):
        hit = (back_mask[..., 0:1] == 255).astype(np.uint8)
        return back * hit + den * (1 - hit)

    for ii, bpart in enumerate(RP.PARTS):
        blank = np.zeros((h, w, 3), np.uint8)
        p_img, p_stick, p_mask = blank, blank, blank
        m_up, _ = PR.crop_matrices(upper_kp, bpart, o_w, o_h, box_factor)
        m_lo, _ = PR.crop_matrices(lower_kp, bpart, o_w, o_h, box_factor)
        _, m_inv = PR.crop_matrices(person_kp, bpart, o_w, o_h, box_factor)
        source = (m_up, upper_img, upper_pose, upper_mask) if ii < UPPER_PARTS else (m_lo, lower_img, lower_pose, lower_mask)
        if source[0] is not None:
            p_img, p_stick, p_mask = (RP.warp_perspective(s, source[0], (w, h), RP.BORDER_REPLICATE) for s in source[1:])
        if m_inv is not None:
            back = RP.warp_perspective(p_img, m_inv, (o_w, o_h), RP.BORDER_CONSTANT)
            back_mask = RP.warp_perspective(p_mask, m_inv, (o_w, o_h), RP.BORDER_CONSTANT)
            if ii < UPPER_PARTS:
                den_u = put(den_u, back, PR.erode(back_mask, ERODE))
            else:
                den_l_plain = put(den_l_plain, back, back_mask)
                if not own_lower:
                    den_l_eroded = put(den_l_eroded, back, PR.erode(back_mask, ERODE))
        imgs.append(p_img)
        sticks.append(p_stick)
        masks.append(p_mask)
    cat = lambda xs: np.concatenate(xs, axis=2)
    return cat(imgs), cat(sticks), cat(masks), den_u, den_l_plain if own_lower else den_l_eroded, den_l_plain, den_l_eroded


def load_outfit(raw):
    """One raw outfit (a dict of UvitonOutfits_256_test) -> the uint8 stages, named as ``tryon_pairs_ref.load_pair`` names them
    (``clothes_stick``: the upper garment's owner's stick figure) with ``lower_stick``, and the two lower composites of
    ``normalize_outfit`` as ``lower_plain`` / ``lower_eroded``.  L is P where the two names are the same, the data set's rule."""
    image, pose, parsing, kp = PR.person_stages(raw['image'], raw['parsing'], raw['keypoints'])
    palm = PR.palm_mask(kp, parsing[..., 0])[..., None]
    head = sum((parsing == v).astype(np.uint8) for v in (1, 4, 2, 13))
    shoes = sum((parsing == v).astype(np.uint8) for v in (18, 19))
    retain_img = image * (palm + head + shoes)
    u_image, u_pose, u_parsing, u_kp = PR.person_stages(raw['upper_image'], raw['upper_parsing'], raw['upper_keypoints'])
    l_image, l_pose, l_parsing, l_kp = PR.person_stages(raw['lower_image'], raw['lower_parsing'], raw['lower_keypoints'])
    upper = sum((u_parsing == v).astype(np.uint8) for v in (5, 6, 7))
    lower = sum((l_parsing == v).astype(np.uint8) for v in (9, 12, 6))
    upper_img, lower_img = upper * u_image, lower * l_image
    upper_mask = np.concatenate([upper] * 3, axis=2) * 255
    lower_mask = np.concatenate([lower] * 3, axis=2) * 255
    own_lower = raw['lower_name'] == raw['person_name']
    patches, stick_patches, mask_patches, den_u, den_l, plain, eroded = normalize_outfit(
        upper_img, lower_img, upper_mask, lower_mask, u_pose, l_pose, u_kp, l_kp, kp, own_lower)
    return dict(palm=palm[..., 0], retain_img=retain_img, stick=pose, clothes_stick=u_pose, lower_stick=l_pose, lower_img=lower_img,
                lower_mask=lower_mask, upper_img=upper_img, upper_mask=upper_mask, patches=patches, stick_patches=stick_patches,
                mask_patches=mask_patches, denorm_upper=den_u, denorm_lower=den_l, lower_plain=plain, lower_eroded=eroded, own_lower=own_lower)
