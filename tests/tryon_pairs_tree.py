"""A tiny directory tree in the layout of the reference's try-on TEST set (training/dataset.py:997-1041): the two sub-datasets
with their pair lists (five lines, so a batch of two leaves a partial batch), written with PIL and json.  The pairs carry the
oddities the loader and the preparation must survive: a donor without shoulders or hips (its upper parts are missing while the
person's exist), a person without a knee (thigh fall-back) or an ankle (shin fall-back), an empty ``people``, a wrist beyond the
canvas, a zero-length forearm and label 6 on the person (it belongs to the lower garment at test time)."""
import json
import os

import numpy as np

from tryon_tree import H, W, label_map, person_keypoints

SUBSETS = ('UPT_subset1_256_192', 'UPT_subset2_256_192')
PAIR_LIST = 'test_pairs_front_list_shuffle_0508.txt'
# (sub-dataset, person, clothes): the order the data set must read them in
PAIRS = [('UPT_subset1_256_192', 'p0.jpg', 'c0.jpg'), ('UPT_subset1_256_192', 'p1.jpg', 'c1.jpg'),
         ('UPT_subset1_256_192', 'p2.jpg', 'c2.jpg'), ('UPT_subset2_256_192', 'p3.jpg', 'c3.jpg'),
         ('UPT_subset2_256_192', 'p4.jpg', 'c4.jpg')]


def pair_keypoints(i, rng):
    """(person, donor) key points of pair i."""
    person, donor = person_keypoints(0, rng), person_keypoints(0, rng)
    if i == 0:
        donor[[2, 5, 8, 11], 2] = 0.05                 # donor: no shoulders, no hips -> parts 0..5 missing, the person's exist
        person[12, 2] = 0.0                            # person: no left knee -> the thigh falls back to the hip
    if i == 1:
        person[10, 2] = 0.02                           # person: no right ankle -> the shin falls back to the knee
        donor[7, :2] = (230.5, 140.25)                 # donor: left wrist beyond column 191
    if i == 2:
        person = None                                  # person: empty ``people``
        donor[4, :2] = donor[3, :2]                    # donor: right forearm of length zero
    if i == 3:
        person[4, :2] = (250.25, 120.5)                # person: right wrist beyond the canvas (palm quadrilateral outside)
        donor = None                                   # donor: empty ``people``
    if i == 4:
        person[3, :2] = person[4, :2]                  # person: right forearm of length zero
    return person, donor


def write_person(root, ds, name, kp, rng, shape, block, label_map, any_person, lower_six=False):
    """A person's three files (shared with tryon_512_tree): a blocky random image of ``shape``, the key points (None: an empty
    ``people``) and the label map, drawn around ``any_person(rng)`` where there are no key points."""
    import PIL.Image
    stem = name[:-len('.jpg')]
    h, w = shape
    img = rng.integers(0, 256, [h // block, w // block, 3]).repeat(block, 0).repeat(block, 1).astype(np.uint8)
    PIL.Image.fromarray(img).save(os.path.join(root, ds, 'image', name), quality=95)
    people = [] if kp is None else [{'pose_keypoints_2d': [float(v) for v in kp.reshape(-1)]}]
    with open(os.path.join(root, ds, 'keypoints', stem + '_keypoints.json'), 'w') as f:
        json.dump({'version': 1.3, 'people': people}, f)
    lab = label_map(rng, kp if kp is not None else any_person(rng))
    if lower_six:
        lab[180:215, 60:130] = 6                       # label 6 over the legs: lower garment of the person
        lab[105:140, 75:115] = 6                       # and over the torso
    PIL.Image.fromarray(lab, mode='L').save(os.path.join(root, ds, 'parsing', stem + '_label.png'))


def make_tree(root, seed, subsets, pairs, pair_keypoints, files, person_lower_six=False):
    """The sub-datasets' directories, every pair's person and donor through ``write_person(..., **files)`` (the person with
    ``lower_six`` where ``person_lower_six``) and the pair lists (shared with tryon_512_tree)."""
    rng = np.random.default_rng(seed)
    root = str(root)
    for ds in subsets:
        for sub in ('image', 'keypoints', 'parsing'):
            os.makedirs(os.path.join(root, ds, sub), exist_ok=True)
    lists = {ds: [] for ds in subsets}
    for i, (ds, person, clothes) in enumerate(pairs):
        kp_p, kp_c = pair_keypoints(i, rng)
        write_person(root, ds, person, kp_p, rng, lower_six=person_lower_six, **files)
        write_person(root, ds, clothes, kp_c, rng, **files)
        lists[ds].append('%s %s\n' % (person, clothes))
    for ds in subsets:
        with open(os.path.join(root, ds, PAIR_LIST), 'w') as f:
            f.writelines(lists[ds])
    return root


def make_pair_tree(root, seed=0):
    files = dict(shape=(H, W), block=4, label_map=label_map, any_person=lambda rng: person_keypoints(0, rng))
    return make_tree(root, seed, SUBSETS, PAIRS, pair_keypoints, files, person_lower_six=True)
