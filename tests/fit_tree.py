"""TEST INFRASTRUCTURE ONLY: ragged trees for --fit-people, derived from the tiny trees (tests/tryon_tree.py and its relatives).
``ragged_copy`` copies a tree and gives every person a size of their own: the photograph and the label map resized with PIL,
the joints scaled.  ``host_fitted_copy`` writes the tree a plain run must see to produce what a --fit-people run produces from
the ragged one: every person fitted to the canvas by the numpy statement (tests/fit_ref.py).  Photographs keep their ``.jpg``
names and hold PNG bytes (PIL opens by content), so both trees decode to exactly the arrays written."""
import json
import os
import shutil

import numpy as np
import PIL.Image

import fit_ref as R

# (height, width) factors of the people's own sizes, cycled: the canvas itself, larger, wider than the canvas's shape, smaller
# and narrower, taller
FACTORS = ((1.0, 1.0), (1.5, 1.5), (1.17, 1.3), (0.8, 0.7), (1.3, 1.0), (0.62, 0.62))


def people(root):
    """(image, label map, key points) paths of every person of a tree, sorted."""
    out = []
    for ds in sorted(os.listdir(root)):
        top = os.path.join(root, ds, 'image')
        if not os.path.isdir(top):
            continue
        for folder, _, files in sorted(os.walk(top)):
            for name in sorted(f for f in files if f.endswith('.jpg')):
                rel = os.path.relpath(os.path.join(folder, name), top)
                stem = rel[:-len('.jpg')]
                labels = [os.path.join(root, ds, 'parsing', stem + tail) for tail in ('_label.png', '.png')]
                out.append((os.path.join(top, rel), [p for p in labels if os.path.exists(p)][0],
                            os.path.join(root, ds, 'keypoints', stem + '_keypoints.json')))
    return out


def _channel0(path):
    with PIL.Image.open(path) as img:
        return np.array(img) if img.mode == 'L' else np.ascontiguousarray(np.array(img.convert('RGB'))[..., 2])


def _write(image_path, label_path, kpt_path, image, labels, joints):
    PIL.Image.fromarray(image).save(image_path, format='PNG')
    PIL.Image.fromarray(labels, mode='L').save(label_path, format='PNG')
    with open(kpt_path) as f:
        data = json.load(f)
    if joints is not None:
        data['people'][0]['pose_keypoints_2d'] = [float(v) for v in np.asarray(joints, np.float64).reshape(-1)]
    with open(kpt_path, 'w') as f:
        json.dump(data, f)


def _joints(kpt_path):
    with open(kpt_path) as f:
        data = json.load(f)
    return None if not data['people'] else np.array(data['people'][0]['pose_keypoints_2d'], np.float64).reshape(-1, 3)


def ragged_copy(src, dst, factors=FACTORS):
    """``src`` copied to ``dst`` with person i resized by ``factors[i % len]``; returns the people's sizes."""
    shutil.copytree(str(src), str(dst))
    sizes = []
    for i, (image_path, label_path, kpt_path) in enumerate(people(str(dst))):
        image, labels = np.array(PIL.Image.open(image_path).convert('RGB')), _channel0(label_path)
        h0, w0 = labels.shape
        fh, fw = factors[i % len(factors)]
        h, w = int(round(h0 * fh)), int(round(w0 * fw))
        assert h >= w
        joints = _joints(kpt_path)
        if joints is not None:
            joints[:, 0] *= w / w0
            joints[:, 1] *= h / h0
        _write(image_path, label_path, kpt_path, np.array(PIL.Image.fromarray(image).resize((w, h), PIL.Image.BICUBIC)),
               np.array(PIL.Image.fromarray(labels, mode='L').resize((w, h), PIL.Image.NEAREST)), joints)
        sizes.append((h, w))
    return sizes


def host_fitted_copy(src, dst, canvas, mode, filter):
    """The ragged tree ``src`` copied to ``dst`` with every person fitted to ``canvas`` by the statement."""
    shutil.copytree(str(src), str(dst))
    for image_path, label_path, kpt_path in people(str(dst)):
        image, labels = np.array(PIL.Image.open(image_path).convert('RGB')), _channel0(label_path)
        joints = _joints(kpt_path)
        fitted_image, fitted_labels, fitted_joints, _ = R.fit_person(image, labels, np.zeros([18, 3]) if joints is None else joints, canvas, mode, filter)
        _write(image_path, label_path, kpt_path, fitted_image, fitted_labels, None if joints is None else fitted_joints)


def host_fitted_sample(sample, keys=('',)):
    """A raw sample that carries ``fit`` -> the plain sample of the same people fitted on the host: for every prefix of ``keys``
    the image, label map and key points on the canvas; ``fit`` removed."""
    fit = sample['fit']
    out = {k: v for k, v in sample.items() if k != 'fit'}
    for prefix in keys:
        image, labels, joints, _ = R.fit_person(sample[prefix + 'image'], sample[prefix + 'parsing'], sample[prefix + 'keypoints'], fit['canvas'],
                                                fit['mode'], fit['filter'])
        out.update({prefix + 'image': image, prefix + 'parsing': labels, prefix + 'keypoints': joints})
    return out
