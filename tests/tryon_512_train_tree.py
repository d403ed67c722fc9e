"""A tiny directory tree in the layout of the 512 x 320 TRAINING set (training.dataset.UvitonDatasetFull_512: the four
``*_512_320`` sub-datasets with the training lists, ``train_img_vis`` and ``train_random_mask_acgpn``), written with PIL and
json.  Five people; the three that ``train_img_vis`` lists (enough for a 3 x 3 snapshot grid, one row per region) are the cases
the 512 training kernels can go wrong on:

    p0  every joint, the right arm folded back so that the boxes of its upper arm and forearm overlap under the sleeve: pixels
        where both arm masks of the erase rule are 1;
    p1  no left wrist and no right ankle: a palm segment with present = 0, an invalid forearm part and an invalid shin (this
        set's get_crop has no shin fall-back);
    p2  the right elbow far outside the canvas (Deepfashion's image/train folder).

``erase_masks`` gives the three people erase masks of three sizes; the first holds 254 on a pixel the caller names."""
import os

import numpy as np

from tryon_512_tree import H, W, standing_person
from tryon_pairs_tree import write_person

SUBSETS = ('Zalando_512_320', 'Zalora_512_320', 'Deepfashion_512_320', 'MPV_512_320')
TRAIN_LIST = 'train_pairs_front_list_0508.txt'
# (sub-dataset, list entry): the order the data set must read them in
PERSONS = [('Zalando_512_320', 'p0.jpg'), ('Zalando_512_320', 'p1.jpg'), ('Zalora_512_320', 'z0.jpg'),
           ('Deepfashion_512_320', 'train/p2.jpg'), ('MPV_512_320', 'm0.jpg')]
VIS = ['p1.jpg', 'p2.jpg', 'nowhere.jpg', 'p0.jpg']     # sorted: nowhere (skipped), p0, p1 (Zalando), p2 (Deepfashion)
VIS_INDEX = [0, 1, 3]
ERASE_SIZES = ((512, 512), (256, 192), (37, 23))


def person_keypoints(i, rng):
    kp = standing_person(rng)
    if i == 0:
        kp[4, :2] = (62.5, 138.25)                     # right wrist back up beside the shoulder: the arm's two boxes overlap
    if i == 1:
        kp[7, 2] = 0.05                                # no left wrist: palm segment 1 absent, part 3 invalid
        kp[10, 2] = 0.02                               # no right ankle: part 9 invalid
    if i == 3:
        kp[3, :2] = (-110.5, 215.25)                   # right elbow left of the padded square
    return kp


def label_map(rng, kp):
    """Every label somewhere; an upper garment (5, 7) with sleeves (6) over the elbows, a lower garment (9, 12), hands (14, 15)
    around the wrists."""
    lab = rng.integers(0, 20, [H // 16, W // 16]).repeat(16, 0).repeat(16, 1).astype(np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    lab[200:300, 116:204] = 5
    lab[130:200, 116:160] = 7
    lab[310:420, 110:210] = 9
    lab[420:460, 110:160] = 12
    for j in (3, 6):
        lab[(yy - kp[j, 1]) ** 2 + (xx - kp[j, 0]) ** 2 < 44 ** 2] = 6
    for j, label in ((7, 14), (4, 15)):
        lab[(yy - kp[j, 1]) ** 2 + (xx - kp[j, 0]) ** 2 < 24 ** 2] = label
    return lab


def erase_masks(wrap_pixel=None, seed=0):
    """Three erase masks (uint8, 0 / 255) of ERASE_SIZES: a few random rectangles each, placed on a 512-square scale over the
    body.  ``wrap_pixel`` (y, x) of the padded square: the 512 x 512 mask holds 254 there."""
    rng = np.random.default_rng(seed)
    masks = []
    for h, w in ERASE_SIZES:
        m = np.zeros([h, w], np.uint8)
        for _ in range(3):
            y0, x0 = rng.uniform(0.2, 0.7), rng.uniform(0.3, 0.55)
            dy, dx = rng.uniform(0.04, 0.10), rng.uniform(0.04, 0.10)
            m[int(y0 * h):int((y0 + dy) * h) + 1, int(x0 * w):int((x0 + dx) * w) + 1] = 255
        masks.append(m)
    if wrap_pixel is not None:
        masks[0][wrap_pixel] = 254
    return masks


def make_512_train_tree(root, seed=0):
    import PIL.Image
    rng = np.random.default_rng(seed)
    root = str(root)
    files = dict(shape=(H, W), block=8, label_map=label_map, any_person=standing_person)
    lists = {ds: [] for ds in SUBSETS}
    for i, (ds, entry) in enumerate(PERSONS):
        for sub in ('image', 'keypoints', 'parsing'):
            os.makedirs(os.path.dirname(os.path.join(root, ds, sub, entry)), exist_ok=True)
        write_person(root, ds, entry, person_keypoints(i, rng), rng, **files)
        lists[ds].append('%s %s\n' % (entry, entry.replace('.jpg', '_cloth.jpg')))
    for ds in SUBSETS:
        with open(os.path.join(root, ds, TRAIN_LIST), 'w') as f:
            f.writelines(lists[ds] + ['\n'])           # an empty line: skipped
    os.makedirs(os.path.join(root, 'train_img_vis'))
    for name in VIS:
        PIL.Image.fromarray(np.zeros([8, 8, 3], np.uint8)).save(os.path.join(root, 'train_img_vis', name))
    os.makedirs(os.path.join(root, 'train_random_mask_acgpn'))
    for k, m in enumerate(erase_masks()):
        PIL.Image.fromarray(m, mode='L').save(os.path.join(root, 'train_random_mask_acgpn', 'm%d.png' % k))
    return root
