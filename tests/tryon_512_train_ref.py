"""numpy restatement of the 512 x 320 TRAINING sample (training.tryon_regions.FullBodyRegionBatchBuilder), one sample at a
time.  The reference ships no 512 training set; the rule is this project's own: a sample is the 512 test set's full-body
preparation of the pair (person, person) -- tests/tryon_512_ref.py's ``person_stages``, ``garments`` and
``normalize_region('fullbody')`` -- plus the 256 training set's photograph, ``gt_parsing`` and erase mask, whose code is
tests/tryon_ref.py's (``resize_linear_u8``, the label sums of ``label_masks``, the uint8 ``+=`` of ``erase_mask``).  Only the
glue is new: the eroded masks of the four arm parts, and the fixed pick arm[2] + arm[3] + resized erase mask that
``random.seed(1)`` makes at 256."""
import numpy as np

import tryon_512_ref as FR
import tryon_pairs_ref as PR
import tryon_ref as R
from oracle import ref_patches as RP

ARM_PARTS = (2, 3, 4, 5)


def gt_parsing(parsing):
    """tests/tryon_ref.py label_masks' gt rule on a uint8 label map of any shape."""
    eq = lambda *labels: sum((parsing == v).astype(np.uint8) for v in labels)
    return eq(5, 6, 7) * 1 + eq(9, 12) * 2 + eq(14, 15) * 3 + eq(16, 17) * 4 + eq(10) * 5


def arm_masks(mask_patches, shifted_kp, side, box_factor=2):
    """The eroded 0 / 1 masks [4, S, S] of the arm parts in the upper composite: each part's mask patch warped back with the
    person's M_inv and eroded 5 x 5 before the == 255 test, as normalize_region's ``back`` does; zeros where the part is
    missing."""
    out = np.zeros([4, side, side], np.uint8)
    for j, k in enumerate(ARM_PARTS):
        _, m_inv = FR.crop_matrices(shifted_kp, RP.PARTS[k], side, side, box_factor)
        if m_inv is not None:
            mask = RP.warp_perspective(np.ascontiguousarray(mask_patches[..., 3 * k:3 * k + 3]), m_inv, (side, side), RP.BORDER_CONSTANT)[..., 0:1]
            out[j] = (PR.erode(mask, 5) == 255).astype(np.uint8)[..., 0]
    return out


def erase_mask(arm, acgpn_channel0, side):
    """tests/tryon_ref.py erase_mask with the draws of random.seed(1) written out (arm masks 2 and 3, then the resized mask),
    on a ``side`` square: the += is uint8 and wraps."""
    m = np.zeros((side, side), dtype=np.uint8)
    m += arm[2]
    m += arm[3]
    m += R.resize_linear_u8(acgpn_channel0, side, side)
    return (m > 0).astype(np.uint8)


def person_training_stages(raw):
    """Everything of a raw sample that does not depend on its erase mask: the uint8 stages under the 256 builder's names."""
    image, pose, parsing, kp = FR.person_stages(raw['image'], raw['parsing'], raw['keypoints'])
    side = image.shape[0]
    shoes = sum((parsing == v).astype(np.uint8) for v in (18, 19))
    head = sum((parsing == v).astype(np.uint8) for v in (1, 2, 4, 13))
    palm = FR.palm_mask(kp, parsing[..., 0])
    retain_mask = (shoes + palm[..., None] + head)[..., 0]
    ui, li, um, lm = FR.garments(image, parsing)
    norm_img, norm_lower, masks, masks_l, den_u, den_l = FR.normalize_region('fullbody', ui, li, um, lm, kp, kp)
    m_invs = np.zeros([10, 3, 3], np.float32)
    for k, part in enumerate(RP.PARTS):
        _, m_inv = FR.crop_matrices(kp, part, side, side)
        if m_inv is not None:
            m_invs[k] = m_inv.astype(np.float32)
    return dict(image=image, stick=pose, palm=palm, retain_mask=retain_mask, gt_parsing=gt_parsing(parsing[..., 0]), upper_img=ui,
                lower_img=li, upper_mask=um, lower_mask=lm, norm_img=norm_img, norm_img_lower=norm_lower, norm_clothes_mask=masks,
                norm_clothes_mask_lower=masks_l, denorm_upper=den_u, denorm_lower=den_l, arm_masks=arm_masks(masks, kp, side), M_invs=m_invs)


def erased(stages, acgpn_channel0):
    """(erase [S, S], denorm_upper and denorm_lower with the erased pixels zeroed)."""
    erase = erase_mask(stages['arm_masks'], acgpn_channel0, stages['image'].shape[0])
    keep = (1 - erase)[..., None]
    return erase, stages['denorm_upper'] * keep, stages['denorm_lower'] * keep


def training_tensors(stages_list, erase_masks, device):
    """The nine tensors of FullBodyBatch.KEYS for a batch, the float expressions evaluated by torch on ``device`` as the
    reference loop does (x / 127.5 - 1; retain = real * mask - (1 - mask) with the uint8 mask)."""
    import torch
    chw = lambda a: a.transpose(2, 0, 1)
    per = []
    for st, em in zip(stages_list, erase_masks):
        _, du, dl = erased(st, em)
        du, dl = chw(du), chw(dl)
        per.append(dict(real=chw(st['image']), pose=chw(st['stick']), ni=chw(st['norm_img']), nl=chw(st['norm_img_lower']), du=du, dl=dl,
                        gt=st['gt_parsing'][None], dum=(np.sum(du, axis=0, keepdims=True) > 0).astype(np.uint8),
                        dlm=(np.sum(dl, axis=0, keepdims=True) > 0).astype(np.uint8), retain=st['retain_mask'][None]))
    b = {k: torch.from_numpy(np.stack([p[k] for p in per])).to(device) for k in per[0]}
    unit = lambda x: x.to(torch.float32) / 127.5 - 1
    real = unit(b['real'])
    head = b['retain'] * real - (1 - b['retain'])
    return dict(real_img=real, style_input=torch.cat([unit(b['ni']), unit(b['nl'])], dim=1), retain=head,
                pose=torch.cat((unit(b['pose']), head), dim=1), denorm_upper_input=unit(b['du']), denorm_lower_input=unit(b['dl']),
                denorm_upper_mask=b['dum'].to(torch.float32), denorm_lower_mask=b['dlm'].to(torch.float32),
                gt_parsing=b['gt'].to(torch.float32))


_CASES = {}


def cases(tree):
    """The three listed people of a tests/tryon_512_train_tree.py tree with erase masks of three sizes, computed once and left
    unchanged: (raw samples, restated stages, wrap pixel).  The wrap pixel is one where both arm masks of person 0 are 1; that
    person's 512 x 512 erase mask holds 254 there, so the uint8 sum wraps to 0 and the pixel is NOT erased."""
    from training.dataset import UvitonDatasetFull_512
    from tryon_512_train_tree import erase_masks
    if tree not in _CASES:
        ds = UvitonDatasetFull_512(tree)
        samples = [ds[i] for i in ds.vis_index]
        stages = [person_training_stages(s) for s in samples]
        both = np.argwhere((stages[0]['arm_masks'][2] == 1) & (stages[0]['arm_masks'][3] == 1) & stages[0]['denorm_upper'].any(axis=2))
        assert len(both) > 0, 'person 0 has no pixel under both arm masks'
        wrap = tuple(int(v) for v in both[len(both) // 2])
        for s, m in zip(samples, erase_masks(wrap)):
            s['erase_mask'] = m
        _CASES[tree] = samples, stages, wrap
    return _CASES[tree]
