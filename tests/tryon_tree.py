"""A tiny directory tree in the layout of the reference's try-on data set (training/dataset.py:426-487), written with PIL and
json: all four sub-datasets (MPV_256_192 with its own label naming), key points with an empty ``people``, joints under 0.1
confidence and joints outside the canvas, ``train_img_vis`` and two ACGPN erase masks of different sizes."""
import json
import os

import numpy as np

H, W = 256, 192
# (sub-dataset, list entry): the order the data set must read them in
PERSONS = [('Zalando_256_192', 'za_0.jpg'), ('Zalando_256_192', 'za_1.jpg'), ('Zalora_256_192', 'zl_0.jpg'),
           ('Deepfashion_256_192', 'train/df_0.jpg'), ('MPV_256_192', 'mpv_0.jpg')]
VIS = ['df_0.jpg', 'nowhere.jpg', 'za_1.jpg']          # sorted: df_0 (Deepfashion), nowhere (skipped), za_1 (Zalando)


def person_keypoints(i, rng):
    """Plausible joints of a standing person, with the per-sample oddities the loader and the kernels must survive."""
    base = np.array([[96, 30], [96, 60], [70, 62], [60, 100], [56, 135], [122, 62], [132, 100], [136, 135], [80, 130], [80, 185],
                     [80, 235], [112, 130], [112, 185], [112, 235], [90, 25], [102, 25], [84, 28], [108, 28]], np.float64)
    kp = np.concatenate([base + rng.uniform(-6, 6, base.shape), rng.uniform(0.3, 1.0, [18, 1])], axis=1)
    if i == 1:
        kp[[3, 9, 15], 2] = 0.05                       # right elbow, right knee, left eye under 0.1
    if i == 2:
        kp[7, :2] = (230.5, 140.25)                    # left wrist beyond column 191 of the canvas
        kp[10, :2] = (-12.75, 250.5)                   # right ankle left of it
    if i == 3:
        kp[4, :2] = kp[3, :2]                          # right forearm of length zero
    return kp


def label_map(rng, kp):
    """Every one of the 20 labels somewhere, hands (14 / 15) around the wrists and elbows so the palm rule has work to do."""
    lab = rng.integers(0, 20, [H // 8, W // 8]).repeat(8, 0).repeat(8, 1).astype(np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for j, label in ((7, 14), (6, 14), (4, 15), (3, 15)):
        lab[(yy - kp[j, 1]) ** 2 + (xx - kp[j, 0]) ** 2 < 18 ** 2] = label
    lab[100:150, 70:120] = 5
    lab[160:220, 70:120] = 9
    return lab


def make_tree(root, seed=0):
    import PIL.Image
    rng = np.random.default_rng(seed)
    root = str(root)
    lists = {}
    for i, (ds, entry) in enumerate(PERSONS):
        stem = entry[:-len('.jpg')]
        for sub in ('image', 'keypoints', 'parsing'):
            os.makedirs(os.path.dirname(os.path.join(root, ds, sub, entry)), exist_ok=True)
        img = rng.integers(0, 256, [H // 4, W // 4, 3]).repeat(4, 0).repeat(4, 1).astype(np.uint8)
        PIL.Image.fromarray(img).save(os.path.join(root, ds, 'image', entry), quality=95)
        kp = person_keypoints(i, rng)
        people = [] if i == 4 else [{'pose_keypoints_2d': [float(v) for v in kp.reshape(-1)]}]
        with open(os.path.join(root, ds, 'keypoints', stem + '_keypoints.json'), 'w') as f:
            json.dump({'version': 1.3, 'people': people}, f)
        lab = label_map(rng, kp)
        label_name = stem + ('.png' if ds == 'MPV_256_192' else '_label.png')
        if i == 0:                                      # a palette PNG: cv2 reads the palette colour's blue, not the index
            pal = PIL.Image.fromarray(lab, mode='P')
            pal.putpalette([v for k in range(256) for v in ((k * 7) % 256, (k * 3) % 256, (255 - 2 * k) % 256)])
            pal.save(os.path.join(root, ds, 'parsing', label_name))
        else:
            PIL.Image.fromarray(lab, mode='L').save(os.path.join(root, ds, 'parsing', label_name))
        lists.setdefault(ds, []).append(entry)
    for ds in ('Zalando_256_192', 'Zalora_256_192', 'Deepfashion_256_192', 'MPV_256_192'):
        with open(os.path.join(root, ds, 'train_pairs_front_list_0508.txt'), 'w') as f:
            f.writelines('%s %s\n' % (e, e.replace('.jpg', '_cloth.jpg')) for e in lists[ds])
    os.makedirs(os.path.join(root, 'train_img_vis'))
    for name in VIS:
        PIL.Image.fromarray(np.zeros([8, 8, 3], np.uint8)).save(os.path.join(root, 'train_img_vis', name))
    os.makedirs(os.path.join(root, 'train_random_mask_acgpn'))
    m0 = np.zeros([H, W], np.uint8)
    m0[60:140, 40:110] = 255
    PIL.Image.fromarray(m0, mode='L').save(os.path.join(root, 'train_random_mask_acgpn', 'm0.png'))
    m1 = np.zeros([128, 96, 3], np.uint8)
    m1[20:90, 30:70] = (255, 255, 255)
    m1[95:110, 10:40] = (0, 0, 200)                     # only the blue channel (channel 0 of cv2's BGR) counts
    PIL.Image.fromarray(m1).save(os.path.join(root, 'train_random_mask_acgpn', 'm1.png'))
    return root
