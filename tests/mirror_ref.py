"""A mirrored person in numpy (include/pasta_hip.h, pasta_tryon_mirror_u8; this project's own rule), written directly
from the statement and one sample at a time.  The tables are written out again here, not imported from the package:

    image      image'[y, x, :] = image[y, W-1-x, :]
    labels     parsing'[y, x] = LUT[parsing[y, W-1-x]]: the identity except 14 <-> 15, 16 <-> 17, 18 <-> 19
    erase      erase'[y, x] = erase[y, w-1-x] on the mask's own h x w
    joints     x' = (W-1) - x for every joint, y and confidence kept; rows (2,5), (3,6), (4,7), (8,11), (9,12), (10,13), (14,15),
               (16,17) exchanged

The mirrored sample is then prepared by the unchanged restatements (tests/tryon_ref.py, tests/tryon_512_train_ref.py)."""
import numpy as np

LABEL_PAIRS = [(14, 15), (16, 17), (18, 19)]
JOINT_PAIRS = [(2, 5), (3, 6), (4, 7), (8, 11), (9, 12), (10, 13), (14, 15), (16, 17)]


def lut():
    table = list(range(256))
    for a, b in LABEL_PAIRS:
        table[a], table[b] = b, a
    return np.array(table, np.uint8)


def mirror_keypoints(kp, width):
    """float64 [18, 3] of one person on an unpadded canvas ``width`` wide."""
    kp = np.asarray(kp, np.float64)
    out = kp.copy()
    for a, b in JOINT_PAIRS:
        out[a], out[b] = kp[b], kp[a]
    out[:, 0] = (width - 1) - out[:, 0]
    return out


def mirror_raw(sample):
    """A raw sample of ``UvitonDatasetFull`` as a mirror shows it; every other key (``raw_idx``) is kept, ``xflip`` is dropped:
    the result is an ordinary unmirrored sample."""
    width = sample['image'].shape[1]
    out = {k: v for k, v in sample.items() if k != 'xflip'}
    out['image'] = np.ascontiguousarray(sample['image'][:, ::-1])
    out['parsing'] = np.ascontiguousarray(lut()[sample['parsing'][:, ::-1]])
    out['keypoints'] = mirror_keypoints(sample['keypoints'], width)
    if 'erase_mask' in sample:
        out['erase_mask'] = np.ascontiguousarray(sample['erase_mask'][:, ::-1])
    return out


def mirror_arrays(image, parsing, erase, erase_hw, flags):
    """The kernel's statement on stacked arrays: image [N, H, W, 3], parsing [N, H, W], erase [N, eh, ew] (or None) with each
    item's own (h, w) in erase_hw; items whose flag is 0 are copied, the table not applied."""
    image_m, parsing_m = image.copy(), parsing.copy()
    erase_m = None if erase is None else erase.copy()
    for n, flag in enumerate(flags):
        if not flag:
            continue
        image_m[n] = image[n][:, ::-1]
        parsing_m[n] = lut()[parsing[n][:, ::-1]]
        if erase is not None:
            h, w = erase_hw[n]
            erase_m[n, :h, :w] = erase[n, :h, :w][:, ::-1]
    return image_m, parsing_m, erase_m
