"""A directory tree in the layout of the reference's training set (training/dataset.py:426-487) whose ``train_img_vis`` lists
seven people, enough for a 6 x 6 snapshot grid (gap = 2: every branch of the grid's source rule is taken).  The people are
tests/tryon_tree.py's: joints under 0.1 confidence (a missing part matrix), a right forearm of length zero and joints outside
the canvas are among the listed ones.  Every person wears an upper and a lower garment of their own shape."""
import json
import os

import numpy as np

from tryon_tree import H, W, label_map, person_keypoints

# (sub-dataset, list entry, the oddity index of tryon_tree.person_keypoints); Zalando and Deepfashion people can be listed
PERSONS = [('Zalando_256_192', 'za_0.jpg', 0), ('Zalando_256_192', 'za_1.jpg', 1), ('Zalando_256_192', 'za_2.jpg', 2),
           ('Zalando_256_192', 'za_3.jpg', 3), ('Zalando_256_192', 'za_4.jpg', 5), ('Zalora_256_192', 'zl_0.jpg', 6),
           ('Deepfashion_256_192', 'train/df_0.jpg', 7), ('Deepfashion_256_192', 'train/df_1.jpg', 8), ('MPV_256_192', 'mpv_0.jpg', 9)]
# sorted, the first six listed are df_0, df_1, za_0, za_1 (missing joints), za_2 (joints off the canvas), za_3 (zero-length forearm)
VIS = ['za_1.jpg', 'za_2.jpg', 'za_3.jpg', 'za_0.jpg', 'za_4.jpg', 'df_0.jpg', 'df_1.jpg', 'nowhere.jpg']
VIS_COUNT = 7               # 'nowhere.jpg' is in no sub-dataset and is skipped


def make_tree(root, seed=3):
    import PIL.Image
    rng = np.random.default_rng(seed)
    root = str(root)
    lists = {}
    for ds, entry, oddity in PERSONS:
        stem = entry[:-len('.jpg')]
        for sub in ('image', 'keypoints', 'parsing'):
            os.makedirs(os.path.dirname(os.path.join(root, ds, sub, entry)), exist_ok=True)
        img = rng.integers(0, 256, [H // 4, W // 4, 3]).repeat(4, 0).repeat(4, 1).astype(np.uint8)
        PIL.Image.fromarray(img).save(os.path.join(root, ds, 'image', entry), quality=95)
        kp = person_keypoints(oddity, rng)
        with open(os.path.join(root, ds, 'keypoints', stem + '_keypoints.json'), 'w') as f:
            json.dump({'version': 1.3, 'people': [{'pose_keypoints_2d': [float(v) for v in kp.reshape(-1)]}]}, f)
        lab = label_map(rng, kp)
        # garments of the person's own extent, so that a swapped garment differs from the person's own
        a, b = rng.integers(0, 30, 2)
        lab[90 + a // 2:150, 60 + b // 3:130 - a // 3] = 5
        lab[150:230 - b, 62 + a // 3:128 - b // 3] = 9
        label_name = stem + ('.png' if ds == 'MPV_256_192' else '_label.png')
        PIL.Image.fromarray(lab, mode='L').save(os.path.join(root, ds, 'parsing', label_name))
        lists.setdefault(ds, []).append(entry)
    for ds in lists:
        with open(os.path.join(root, ds, 'train_pairs_front_list_0508.txt'), 'w') as f:
            f.writelines('%s %s\n' % (e, e.replace('.jpg', '_cloth.jpg')) for e in lists[ds])
    os.makedirs(os.path.join(root, 'train_img_vis'))
    for name in VIS:
        PIL.Image.fromarray(np.zeros([8, 8, 3], np.uint8)).save(os.path.join(root, 'train_img_vis', name))
    os.makedirs(os.path.join(root, 'train_random_mask_acgpn'))
    m0 = np.zeros([H, W], np.uint8)
    m0[60:140, 40:110] = 255
    PIL.Image.fromarray(m0, mode='L').save(os.path.join(root, 'train_random_mask_acgpn', 'm0.png'))
    return root
