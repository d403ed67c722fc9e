"""A tiny directory tree in the layout of the reference's 512 x 320 try-on TEST set (training/dataset.py:1542-1563): the four
sub-datasets with their pair lists (five lines, so a batch of two leaves a partial batch), 512 x 320 images, written with PIL
and json.  The pairs carry the oddities the loader and the preparation must survive: a donor without shoulders or hips (its
torso, head and upper arms are missing while the person's exist), a person without an ankle (the shin is invalid here, where
the 256 test set would fall back to the knee), a person without a knee (the thigh falls back to row 511), an empty ``people``
on either side, a wrist beyond the canvas, a zero-length forearm, and hands (labels 14, 15) around the wrists and elbows."""
import numpy as np

from tryon_pairs_tree import PAIR_LIST, make_tree, write_person

H, W = 512, 320
SUBSETS = ('Zalando_512_320', 'Zalora_512_320', 'Deepfashion_512_320', 'MPV_512_320')
# (sub-dataset, person, clothes): the order the data set must read them in
PAIRS = [('Zalando_512_320', 'p0.jpg', 'c0.jpg'), ('Zalando_512_320', 'p1.jpg', 'c1.jpg'), ('Zalora_512_320', 'p2.jpg', 'c2.jpg'),
         ('Deepfashion_512_320', 'p3.jpg', 'c3.jpg'), ('MPV_512_320', 'p4.jpg', 'c4.jpg')]


def standing_person(rng):
    """Plausible joints of a standing person on the 512 x 320 canvas, [18, 3]."""
    base = np.array([[160, 60], [160, 120], [116, 124], [100, 200], [93, 270], [204, 124], [220, 200], [227, 270], [133, 260], [133, 370],
                     [133, 470], [187, 260], [187, 370], [187, 470], [150, 50], [170, 50], [140, 56], [180, 56]], np.float64)
    return np.concatenate([base + rng.uniform(-10, 10, base.shape), rng.uniform(0.3, 1.0, [18, 1])], axis=1)


def pair_keypoints(i, rng):
    """(person, donor) key points of pair i; None = an empty ``people`` list."""
    person, donor = standing_person(rng), standing_person(rng)
    if i == 0:
        donor[[2, 5, 8, 11], 2] = 0.05                 # donor: no shoulders, no hips -> parts 0, 1, 2, 4, 6, 8 missing, the person's exist
    if i == 1:
        person[10, 2] = 0.02                           # person: no right ankle -> part 9 is invalid (no shin fall-back here)
        donor[7, :2] = (380.5, 280.25)                 # donor: left wrist beyond column 319
    if i == 2:
        person[12, 2] = 0.0                            # person: no left knee -> the thigh falls back to the hip and row 511
        donor[4, :2] = donor[3, :2]                    # donor: right forearm of length zero
    if i == 3:
        person = None                                  # person: empty ``people``
    if i == 4:
        person[4, :2] = (400.25, 240.5)                # person: right wrist beyond the canvas (palm quadrilateral outside)
        donor = None                                   # donor: empty ``people``
    return person, donor


def label_map(rng, kp):
    """Every one of the 20 labels somewhere, hands (14 / 15) around the wrists and elbows so the palm rule has work to do, both
    garments over the body."""
    lab = rng.integers(0, 20, [H // 16, W // 16]).repeat(16, 0).repeat(16, 1).astype(np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    lab[200:300, 116:204] = 5
    lab[130:200, 116:160] = 7
    lab[310:420, 110:210] = 9
    lab[420:460, 110:160] = 12
    for j, label in ((7, 14), (6, 14), (4, 15), (3, 15)):
        lab[(yy - kp[j, 1]) ** 2 + (xx - kp[j, 0]) ** 2 < 34 ** 2] = label
    return lab


def make_512_tree(root, seed=0):
    files = dict(shape=(H, W), block=8, label_map=label_map, any_person=standing_person)
    return make_tree(root, seed, SUBSETS, PAIRS, pair_keypoints, files)
