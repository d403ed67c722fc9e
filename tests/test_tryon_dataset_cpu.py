"""training/dataset.py: UvitonDatasetFull reads the reference's directory layout (file order, naming variants, _vis_index,
max_size, erase masks) and returns the raw sample the GPU builder takes; collate pads erase masks of different sizes."""
import os

import numpy as np
import pytest

import dnnlib
from tryon_tree import PERSONS, make_tree


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return make_tree(tmp_path_factory.mktemp('tryon'))


def _open(tree, **kw):
    return dnnlib.util.construct_class_by_name(class_name='training.dataset.UvitonDatasetFull', path=tree, **kw)


def test_file_order_naming_and_vis_index(tree):
    ds = _open(tree)
    assert len(ds) == len(PERSONS) and ds.resolution == 256 and ds.image_shape == [3, 256, 256]
    assert ds._image_fnames == [os.path.join(d, 'image', e) for d, e in PERSONS]
    assert ds._kpt_fnames[3] == os.path.join('Deepfashion_256_192', 'keypoints', 'train/df_0_keypoints.json')
    assert ds._parsing_fnames[0] == os.path.join('Zalando_256_192', 'parsing', 'za_0_label.png')
    assert ds._parsing_fnames[4] == os.path.join('MPV_256_192', 'parsing', 'mpv_0.png')
    assert ds.vis_index == [3, 1]                    # df_0 (Deepfashion image/train/), za_1 (Zalando); the unknown name is skipped
    assert ds._mask_acgpn_numbers == 2
    assert ds.name == os.path.basename(tree)


def test_max_size_and_xflip(tree):
    ds = _open(tree, max_size=3, random_seed=0)
    idx = np.arange(5)
    np.random.RandomState(0).shuffle(idx)
    assert len(ds) == 3 and list(ds._raw_idx) == sorted(idx[:3])
    with pytest.raises(ValueError):
        _open(tree, xflip=True)
    with pytest.raises(IOError):
        _open(tree, resolution=512)


def test_raw_sample(tree):
    import PIL.Image
    ds = _open(tree)
    for i in range(len(ds)):
        s = ds[i]
        assert s['image'].dtype == np.uint8 and s['image'].shape == (256, 192, 3)
        assert s['parsing'].dtype == np.uint8 and s['parsing'].shape == (256, 192)
        assert s['keypoints'].dtype == np.float64 and s['keypoints'].shape == (18, 3)
        assert s['erase_mask'].dtype == np.uint8 and s['erase_mask'].ndim == 2
        assert s['raw_idx'] == i
    assert not ds[4]['keypoints'].any()              # empty `people`
    assert ds[1]['keypoints'][3, 2] == pytest.approx(0.05)
    # the palette label map reads as the palette colour's blue component, like channel 0 of cv2.imread
    with PIL.Image.open(os.path.join(tree, ds._parsing_fnames[0])) as im:
        index = np.array(im)
    assert np.array_equal(ds[0]['parsing'], ((255 - 2 * index.astype(np.int64)) % 256).astype(np.uint8))
    with PIL.Image.open(os.path.join(tree, ds._parsing_fnames[1])) as im:
        assert np.array_equal(ds[1]['parsing'], np.array(im))
    # erase masks: file raw_idx % count in os.listdir order, channel 0 (blue) of the file
    names = os.listdir(os.path.join(tree, 'train_random_mask_acgpn'))
    for i in range(3):
        m = ds[i]['erase_mask']
        assert m.shape == {'m0.png': (256, 192), 'm1.png': (128, 96)}[names[i % 2]]
    m1 = ds[names.index('m1.png')]['erase_mask']
    assert m1[100, 20] == 200 and m1[50, 50] == 255 and m1[0, 0] == 0


def test_collate_pads_erase_masks(tree):
    from training.dataset import collate
    ds = _open(tree)
    b = collate([ds[i] for i in range(3)])
    assert tuple(b['image'].shape) == (3, 256, 192, 3) and tuple(b['parsing'].shape) == (3, 256, 192)
    assert tuple(b['keypoints'].shape) == (3, 18, 3) and tuple(b['erase_masks'].shape) == (3, 256, 192)
    for i in range(3):
        h, w = (int(v) for v in b['erase_hw'][i])
        assert np.array_equal(b['erase_masks'][i, :h, :w].numpy(), ds[i]['erase_mask'])
        assert not b['erase_masks'][i, h:].any() and not b['erase_masks'][i, :, w:].any()
    assert b['raw_idx'].tolist() == [0, 1, 2]
