"""Outfits at 512 x 320 on the host: the list format of ``training.dataset.UvitonOutfits_512_test`` on the tiny 512 tree
(tests/tryon_512_tree.py), its refusals, the raw outfit and ``collate_outfits``' deduplicated people stack.  No GPU."""
import os

import numpy as np
import pytest
import torch

from tryon_512_tree import PAIRS, make_512_tree


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return make_512_tree(tmp_path_factory.mktemp('outfits512_cpu'))


def _name(i, who):
    """'<sub-dataset>/<file>' of the person ('p') or the donor ('c') of the tree's pair i, as a list names it."""
    ds, person, clothes = PAIRS[i]
    return '%s/%s' % (ds, person if who == 'p' else clothes)


def _path(name):
    ds, fname = name.split('/')
    return os.path.join(ds, 'image', fname)


def _dataset(tree, tmp_path, text, **kw):
    from training.dataset import UvitonOutfits_512_test
    listing = tmp_path / 'outfits.txt'
    listing.write_text(text)
    return UvitonOutfits_512_test(tree, str(listing), **kw), str(listing)


def test_a_list_is_parsed_line_by_line(tree, tmp_path):
    from training.dataset import UvitonDatasetFull_512_test
    p0, c0, c1, c2, c3 = _name(0, 'p'), _name(0, 'c'), _name(1, 'c'), _name(2, 'c'), _name(3, 'c')
    text = '%s %s %s\n\n   \n%s\t%s   %s  \n%s - -\n%s - %s\n%s %s -\n' % (p0, c0, c1, p0, c2, c3, p0, p0, c1, p0, c2)
    ds, _ = _dataset(tree, tmp_path, text, use_labels=True, max_size=None, xflip=False)
    assert len(ds) == 5 and ds.image_shape == [3, 512, 512] and ds.resolution == 512
    pairs = UvitonDatasetFull_512_test(path=tree, change_region='fullbody')
    by_name = {}
    for i in range(len(pairs)):
        raw = pairs[i]
        by_name[raw['person_name']] = (raw['image'], raw['parsing'], raw['keypoints'])
        by_name[raw['clothes_name']] = (raw['clothes_image'], raw['clothes_parsing'], raw['clothes_keypoints'])
    want = [(p0, c0, c1), (p0, c2, c3), (p0, p0, p0), (p0, p0, c1), (p0, c2, p0)]   # c2 and c3: two other sub-datasets than p0's
    assert {n.split('/')[0] for n in (p0, c2, c3)} == {'Zalando_512_320', 'Zalora_512_320', 'Deepfashion_512_320'}
    for i, names in enumerate(want):
        raw = ds[i]
        assert raw['raw_idx'] == i
        assert sorted(raw) == sorted(['image', 'parsing', 'keypoints', 'upper_image', 'upper_parsing', 'upper_keypoints', 'lower_image',
                                      'lower_parsing', 'lower_keypoints', 'person_name', 'upper_name', 'lower_name', 'raw_idx'])
        for role, prefix, name in zip(('person', 'upper', 'lower'), ('', 'upper_', 'lower_'), names):
            assert raw[role + '_name'] == _path(name), (i, role)
            image, parsing, kp = by_name[_path(name)]                # resolved exactly as the pair lists' names are
            assert raw[prefix + 'image'].dtype == np.uint8 and raw[prefix + 'image'].shape == (512, 320, 3)
            assert np.array_equal(raw[prefix + 'image'], image) and np.array_equal(raw[prefix + 'parsing'], parsing)
            assert raw[prefix + 'keypoints'].dtype == np.float64 and np.array_equal(raw[prefix + 'keypoints'], kp)
    # '-' is the person's own arrays, and a file named twice on a line is decoded once
    own = ds[2]
    assert own['upper_image'] is own['image'] and own['lower_parsing'] is own['parsing'] and own['upper_keypoints'] is own['keypoints']
    ds2, _ = _dataset(tree, tmp_path, '%s %s %s\n' % (p0, c0, c0))
    twice = ds2[0]
    assert twice['upper_image'] is twice['lower_image'] and twice['upper_image'] is not twice['image']


def test_every_refusal_names_the_file_and_the_line(tree, tmp_path):
    p0, c0 = _name(0, 'p'), _name(0, 'c')
    good = '%s %s %s\n' % (p0, c0, c0)
    cases = [(good + '\n' + '%s %s\n' % (p0, c0), 3, 'fields'),                      # two fields, after a blank line: line 3
             (good + '%s %s %s %s\n' % (p0, c0, c0, c0), 2, 'fields'),               # four fields
             ('%s\n' % p0, 1, 'fields'),
             (good + good + '%s UPT_subset1_256_192/c0.jpg %s\n' % (p0, c0), 3, 'sub-dataset'),
             (good + '%s %s p9.jpg\n' % (p0, c0), 2, 'sub-dataset'),                 # no sub-dataset at all
             ('\n\n- %s %s\n' % (c0, c0), 3, 'person')]
    for text, line, word in cases:
        with pytest.raises(ValueError) as e:
            _dataset(tree, tmp_path, text)
        message = str(e.value)
        assert str(tmp_path / 'outfits.txt') in message and 'line %d' % line in message and word in message, (text, message)
    with pytest.raises(IOError):
        _dataset(tree, tmp_path, '\n\n')                             # no outfit at all
    ds, _ = _dataset(tree, tmp_path, good + '%s Zalora_512_320/nobody.jpg -\n' % p0)
    assert len(ds) == 2 and ds[0]['raw_idx'] == 0
    with pytest.raises(IOError):                                     # a missing file: at load, as the pairs' data set
        ds[1]
    with pytest.raises(IOError):
        _dataset(str(tmp_path / 'missing'), tmp_path, good)
    with pytest.raises(IOError, match='resolution'):
        _dataset(tree, tmp_path, good, resolution=256)


def test_collate_stacks_every_distinct_person_once(tree, tmp_path):
    from training.dataset import collate_outfits
    p0, p1, c0, c1 = _name(0, 'p'), _name(1, 'p'), _name(0, 'c'), _name(1, 'c')
    # p1 is a person in line 2 and line 0's lower donor; c0 serves lines 0 and 2; line 1 keeps both garments
    text = '%s %s %s\n%s - -\n%s %s -\n%s %s %s\n' % (p0, c0, p1, p0, p1, c0, c1, p1, c0)
    ds, _ = _dataset(tree, tmp_path, text)
    samples = [ds[i] for i in range(len(ds))]
    b = collate_outfits(samples)
    assert b['people_name'] == [_path(n) for n in (p0, c0, p1, c1)]              # first appearance: person, upper, lower per line
    assert b['person_idx'].tolist() == [0, 0, 2, 3] and b['upper_idx'].tolist() == [1, 0, 1, 2] and b['lower_idx'].tolist() == [2, 0, 2, 1]
    for k in ('person_idx', 'upper_idx', 'lower_idx', 'raw_idx'):
        assert b[k].dtype == torch.int64 and tuple(b[k].shape) == (4,)
    assert b['raw_idx'].tolist() == [0, 1, 2, 3]
    assert b['people_image'].dtype == torch.uint8 and tuple(b['people_image'].shape) == (4, 512, 320, 3)
    assert b['people_parsing'].dtype == torch.uint8 and tuple(b['people_parsing'].shape) == (4, 512, 320)
    assert b['people_keypoints'].dtype == torch.float64 and tuple(b['people_keypoints'].shape) == (4, 18, 3)
    for role, prefix in (('person', ''), ('upper', 'upper_'), ('lower', 'lower_')):
        assert b[role + '_name'] == [s[role + '_name'] for s in samples]
        for i, s in enumerate(samples):
            j = int(b[role + '_idx'][i])
            assert b['people_name'][j] == s[role + '_name']
            assert np.array_equal(b['people_image'][j].numpy(), s[prefix + 'image'])
            assert np.array_equal(b['people_parsing'][j].numpy(), s[prefix + 'parsing'])
            assert np.array_equal(b['people_keypoints'][j].numpy(), s[prefix + 'keypoints'])
    # a batch that is one '- -' line: one person
    one = collate_outfits(samples[1:2])
    assert one['people_name'] == [_path(p0)] and one['person_idx'].tolist() == one['upper_idx'].tolist() == one['lower_idx'].tolist() == [0]
    assert tuple(one['people_image'].shape) == (1, 512, 320, 3) and one['raw_idx'].tolist() == [1]
    # two lines that name the same four people in other roles
    full = collate_outfits([samples[0], samples[3]])
    assert len(full['people_name']) == 4 and full['person_idx'].tolist() == [0, 3] and full['lower_idx'].tolist() == [2, 1]


def test_the_entries_are_declared_typed_and_exported():
    import re
    from conftest import ROOT
    from torch_utils import custom_ops
    header = open(os.path.join(ROOT, 'include', 'pasta_hip.h')).read()
    lib = custom_ops.get_plugin()
    for name, args in (('pasta_tryon_outfit_masks_u8', 17), ('pasta_tryon_outfit_assemble', 18)):
        assert re.search(r'\bint %s\(' % name, header) and hasattr(lib, name), name
        assert name in custom_ops.ABI and len(custom_ops.ABI[name][1]) == args
    assert lib.pasta_abi_version() == custom_ops.EXPECTED_ABI == 22


def test_the_merged_entries_refuse_bad_arguments_before_any_launch():
    """The host guards of the ABI-22 try-on entries: pointers are the never-dereferenced value 1, and every call is refused with
    the entry's own text before anything is launched."""
    import ctypes
    from torch_utils import custom_ops
    lib = custom_ops.get_plugin()

    def refused(status, text):
        assert status != 0 and text in lib.pasta_last_error(), lib.pasta_last_error()

    def assemble(slots, photographs):
        outs = (ctypes.c_void_p * 10)(*slots)
        return lib.pasta_tryon_outfit_assemble(*photographs, *[1] * 6, outs, 2, 20, 12, 3, 3, 5, 5, None)
    refused(assemble([None] + [1] * 9, [1, 1, 1]), b'tryon_outfit_assemble: outputs 0 and 1')          # slot 0 null, slot 1 set
    refused(assemble([1] * 10, [1, 1, None]), b'tryon_outfit_assemble: null photograph')               # slot 9 without lower_donor_image
    refused(assemble([1] * 10, [None, 1, 1]), b'tryon_outfit_assemble: null photograph')               # slot 0 without image
    refused(assemble([1] * 4 + [None] + [1] * 5, [1, 1, 1]), b'tryon_outfit_assemble: output 4 is null')
    refused(assemble([None, None] + [1] * 8, [None, None, 1]), b'output 9 needs them')                 # clothes_lower without image / clothes
    refused(lib.pasta_patch_composite_eroded_u8(*[1] * 6, 3, 4, 5, 5, 64, 48, 9, None, None), b'patch_composite_eroded_u8: radius 9 (0..8)')
    refused(lib.pasta_tryon_outfit_masks_u8(*[1] * 12, 2, 20, 12, 2, None), b'tryon_outfit_masks_u8: six_is_lower 2')
    refused(lib.pasta_pose_stickman_u8(*[1] * 3, 2, 20, 12, 0, 2, None), b'pose_stickman_u8: thickness 0, radius 2')
    refused(lib.pasta_palm_mask_u8(*[1] * 4, 1, 520, 320, 35, 20, None), b'palm_mask_u8: bad shape')


def test_cli_lists_the_options_and_refuses_outfits_with_a_region(tmp_path):
    import subprocess
    import sys
    from conftest import ROOT
    cli = os.path.join(ROOT, 'pasta-gan_amd', 'test_512.py')
    run = lambda *args: subprocess.run([sys.executable, cli, *args], capture_output=True, text=True, timeout=120, cwd=ROOT)
    r = run('--help')
    assert r.returncode == 0 and '--outfits' in r.stdout and '--scores' in r.stdout and '--change-region' in r.stdout, r.stderr
    r = run('--network', str(tmp_path / 'none.pkl'), '--outdir', str(tmp_path / 'out'), '--dataroot', str(tmp_path), '--outfits',
            str(tmp_path / 'outfits.txt'), '--change-region', 'fullbody')
    assert r.returncode != 0 and '--outfits' in r.stderr and '--change-region' in r.stderr, (r.returncode, r.stderr)
    assert not (tmp_path / 'out').exists()
