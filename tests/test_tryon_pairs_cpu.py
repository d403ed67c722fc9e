"""The try-on TEST pairs on the host: the loader of UvitonDatasetV19_test on a tiny tree (tests/tryon_pairs_tree.py), the rules
where the test set differs from the training set (erosion, the 15 x 15 forearm box, float64 shifting, the shin fall-back) on
constructed cases, and the command line of pasta-gan_amd/test.py.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

import tryon_pairs_ref as PR
import tryon_ref as R
from conftest import ROOT
from oracle import ref_patches as RP
from tryon_pairs_tree import PAIRS, make_pair_tree

CLI = os.path.join(ROOT, 'pasta-gan_amd', 'test.py')


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return make_pair_tree(tmp_path_factory.mktemp('pairs'))


def test_loader_reads_the_pair_lists_in_order(tree):
    from training.dataset import UvitonDatasetV19_test, collate_pairs
    ds = UvitonDatasetV19_test(path=tree, use_labels=True, max_size=None, xflip=False)
    assert len(ds) == len(PAIRS) and ds.image_shape == [3, 256, 256] and ds.vis_index == list(range(64))
    for i, (sub, person, clothes) in enumerate(PAIRS):
        raw = ds[i]
        assert raw['person_name'] == sub + '/image/' + person and raw['clothes_name'] == sub + '/image/' + clothes
        assert raw['image'].shape == raw['clothes_image'].shape == (256, 192, 3) and raw['image'].dtype == np.uint8
        assert raw['parsing'].shape == raw['clothes_parsing'].shape == (256, 192) and raw['parsing'].dtype == np.uint8
        assert raw['keypoints'].dtype == raw['clothes_keypoints'].dtype == np.float64 and raw['keypoints'].shape == (18, 3)
    # the MPV rule (:1030-1033) names label maps <stem>_label.png outside MPV_256_192
    assert ds._parsing_fnames[0] == os.path.join('UPT_subset1_256_192', 'parsing', 'p0_label.png')
    assert ds._clothes_kpt_fnames[4] == os.path.join('UPT_subset2_256_192', 'keypoints', 'c4_keypoints.json')
    assert not ds[2]['keypoints'].any() and not ds[3]['clothes_keypoints'].any()          # empty ``people``
    assert (ds[0]['parsing'] == 6).any()
    batch = collate_pairs([ds[i] for i in (3, 4)])
    assert tuple(batch['image'].shape) == (2, 256, 192, 3) and tuple(batch['clothes_parsing'].shape) == (2, 256, 192)
    assert batch['person_name'] == [os.path.join('UPT_subset2_256_192', 'image', p) for p in ('p3.jpg', 'p4.jpg')]
    assert batch['raw_idx'].tolist() == [3, 4]


def test_loader_refuses_a_label_map_of_another_size(tmp_path):
    import PIL.Image
    from training.dataset import UvitonDatasetV19_test
    root = make_pair_tree(tmp_path)
    PIL.Image.fromarray(np.zeros([128, 96], np.uint8), mode='L').save(os.path.join(root, 'UPT_subset2_256_192', 'parsing', 'c4_label.png'))
    ds = UvitonDatasetV19_test(path=root)
    ds[3]
    with pytest.raises(IOError, match='label map'):
        ds[4]


@pytest.mark.parametrize('k', [5, 4, 3])
def test_brute_force_erode_is_scipys_minimum_filter(k):
    from scipy import ndimage
    rng = np.random.default_rng(k)
    img = np.where(rng.uniform(size=[40, 33, 3]) < 0.9, 255, rng.integers(0, 256, [40, 33, 3])).astype(np.uint8)
    ref = np.stack([ndimage.minimum_filter(img[..., c], size=k, mode='constant', cval=255) for c in range(3)], axis=2)
    assert np.array_equal(PR.erode(img, k), ref)
    assert (PR.erode(img, k) != img).any()


def test_the_15_box_forearm_palm_differs_from_the_16_box_one():
    """Rule 4: a hand across the forearm's quadrilateral: its pixels 8 columns right of the fill are covered by the 16 x 16 box
    (offsets -8..7, so it reaches 8 to the right) and not by the 15 x 15 one (-7..7)."""
    kp = np.zeros([18, 3])
    kp[[5, 6, 7], :] = [[150, 40, 1], [150, 90, 1], [150, 140, 1]]     # a vertical left arm, already shifted
    kp[[2, 3, 4], 2] = 0
    _, forearm = PR.hand_masks(kp[[5, 6, 7]], 15)
    _, forearm16 = PR.hand_masks(kp[[5, 6, 7]], 16)
    parsing = np.zeros([256, 256], np.uint8)
    parsing[100:130, 100:200] = 14                     # across the forearm, left and right of it
    p15, p16 = PR.palm_mask(kp, parsing, 15), PR.palm_mask(kp, parsing, 16)
    assert (forearm16 != forearm).any() and (p15 != p16).any()
    assert (p15 >= p16).all()                          # the smaller box leaves more of the hand as palm


def _first_double_rounding(rng):
    for _ in range(100000):
        x = rng.uniform(0, 192)
        if np.float32(x + 32.0) != np.float32(x) + np.float32(32):
            return x
    raise AssertionError('no double rounding found')


def test_shifting_in_float64_first_changes_the_quadrilaterals():
    """Rule 6: keypoints[:, 0] += 32 in float64, then float32 (test set), is not float32(x) + 32 (training set)."""
    from training import patch_pipeline as PP
    rng = np.random.default_rng(0)
    kp = np.concatenate([rng.uniform(40, 150, [18, 2]), np.ones([18, 1])], axis=1)
    kp[6, 0] = _first_double_rounding(rng)             # the left elbow: parts 2 and 3
    shifted = kp.copy()
    shifted[:, 0] += 32
    part = PP.BODY_PARTS[2]
    test_quad = PP.part_quadrilateral(shifted, part, 256, x_pad=0)
    train_quad = PP.part_quadrilateral(kp, part, 256)
    assert not np.array_equal(test_quad, train_quad)
    assert np.array_equal(test_quad, RP.part_quadrilateral(shifted, part, 256, x_pad=0))
    assert np.array_equal(train_quad, RP.part_quadrilateral(kp, part, 256))


def test_pair_matrices_equal_the_restatement_and_training_is_unchanged():
    """patch_pipeline.part_matrices(x_pad=0, shin_fallback=True) is get_crop of the test set (the shin falls back to the knee);
    its defaults are still the training set's (no shin fall-back, + 32 in float32)."""
    from training import patch_pipeline as PP
    rng = np.random.default_rng(1)
    kp = np.concatenate([rng.uniform(0, 250, [3, 18, 2]), rng.uniform(0.2, 1, [3, 18, 1])], axis=2)
    kp[0, 10, 2] = 0.05                                # no right ankle: shin from the knee
    kp[1, 13, 2] = 0.05                                # no left ankle
    kp[1, 9, 2] = 0.0                                  # no right knee: thigh from the hip, shin missing
    kp[2, [2, 5], 2] = 0.0                             # no shoulders
    shifted = kp.copy()
    shifted[..., 0] += 32
    fwd, back, valid = PP.part_matrices(shifted, 256, 256, x_pad=0, shin_fallback=True)
    for i in range(3):
        for k, part in enumerate(RP.PARTS):
            m, m_inv = PR.crop_matrices(shifted[i], part, 256, 256)
            assert valid[i, k] == (m is not None), (i, k)
            if m is not None:
                assert np.array_equal(fwd[i, k], m) and np.array_equal(back[i, k], m_inv), (i, k)
    assert valid[0, 9] and valid[1, 7] and not valid[1, 9] and valid[1, 8]
    fwd0, _, valid0 = PP.part_matrices(kp, 256, 256)
    ref = [RP.part_transforms(kp[i], 256, 256) for i in range(3)]
    assert not valid0[0, 9] and not valid0[1, 7]
    for i in range(3):
        for k in range(10):
            assert valid0[i, k] == (ref[i][k][0] is not None) and (not valid0[i, k] or np.array_equal(fwd0[i, k], ref[i][k][0]))


def _cli(*args):
    return subprocess.run([sys.executable, CLI, *args], capture_output=True, text=True, timeout=120, cwd=ROOT)


def test_cli_help_lists_the_reference_options():
    r = _cli('--help')
    assert r.returncode == 0, r.stderr
    for opt in ('--network', '--outdir', '--dataroot', '--batchsize', '--noise-mode', '--trunc', '--seeds', '--class', '--projected-w', '--workers'):
        assert opt in r.stdout, opt


def test_cli_refuses_a_url(tmp_path):
    r = _cli('--network', 'https://example.com/network-snapshot.pkl', '--outdir', str(tmp_path / 'out'), '--dataroot', str(tmp_path))
    assert r.returncode != 0 and 'URL' in r.stderr, (r.returncode, r.stderr)
    assert not (tmp_path / 'out').exists()
    r = _cli('--network', str(tmp_path / 'missing.pkl'), '--outdir', str(tmp_path / 'out'), '--dataroot', str(tmp_path))
    assert r.returncode != 0 and 'not a file' in r.stderr
