"""Outfits for the 256 x 192 model on the host: the list format of ``training.dataset.UvitonOutfits_256_test`` on the tiny test
tree (tests/tryon_pairs_tree.py), its refusals, the raw outfit, ``collate_outfits``' deduplicated people stack on a 256 batch,
a pair, and a collated batch of pairs, taken as the outfits of a change region, the two native entries' declarations and test.py's
two options.  No GPU."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from tryon_pairs_tree import PAIRS, make_pair_tree

CLI = os.path.join(ROOT, 'pasta-gan_amd', 'test.py')


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return make_pair_tree(tmp_path_factory.mktemp('outfits256_cpu'))


def _name(i, who):
    """'<sub-dataset>/<file>' of the person ('p') or the donor ('c') of the tree's pair i, as a list names it."""
    ds, person, clothes = PAIRS[i]
    return '%s/%s' % (ds, person if who == 'p' else clothes)


def _path(name):
    ds, fname = name.split('/')
    return os.path.join(ds, 'image', fname)


def _dataset(tree, tmp_path, text, **kw):
    from training.dataset import UvitonOutfits_256_test
    listing = tmp_path / 'outfits.txt'
    listing.write_text(text)
    return UvitonOutfits_256_test(tree, str(listing), **kw), str(listing)


def test_the_two_outfit_classes_differ_in_class_attributes_only():
    from training import dataset as D
    own = {k for k in vars(D.UvitonOutfits_256_test) if not k.startswith('__')}
    assert own == {'_sub_datasets', '_label_name'} and issubclass(D.UvitonOutfits_256_test, D.UvitonOutfits_512_test)
    assert D.UvitonOutfits_256_test._sub_datasets == D.TEST_SUB_DATASETS == D.UvitonDatasetV19_test._sub_datasets
    label = D.UvitonOutfits_256_test._label_name
    assert label('UPT_subset1_256_192', 'a.jpg') == 'a_label.png' and label('MPV_256_192', 'a.jpg') == 'a.png'        # the 256 set's rule
    assert D.UvitonOutfits_512_test._label_name('MPV_512_320', 'a.jpg') == 'a_label.png'


def test_a_list_is_parsed_line_by_line(tree, tmp_path):
    from training.dataset import UvitonDatasetV19_test
    p0, c0, c1, p3, c3 = _name(0, 'p'), _name(0, 'c'), _name(1, 'c'), _name(3, 'p'), _name(3, 'c')
    text = '%s %s %s\n\n   \n%s\t%s   %s  \n%s - -\n%s - %s\n%s %s -\n' % (p0, c0, c1, p0, c3, p3, p0, p0, c1, p3, c0)
    ds, _ = _dataset(tree, tmp_path, text, use_labels=True, max_size=None, xflip=False)
    assert len(ds) == 5 and ds.image_shape == [3, 256, 256] and ds.resolution == 256
    pairs = UvitonDatasetV19_test(path=tree)
    by_name = {}
    for i in range(len(pairs)):
        raw = pairs[i]
        by_name[raw['person_name']] = (raw['image'], raw['parsing'], raw['keypoints'])
        by_name[raw['clothes_name']] = (raw['clothes_image'], raw['clothes_parsing'], raw['clothes_keypoints'])
    want = [(p0, c0, c1), (p0, c3, p3), (p0, p0, p0), (p0, p0, c1), (p3, c0, p3)]     # p3 and c3: the other sub-dataset than p0's
    assert {n.split('/')[0] for n in (p0, c3)} == {'UPT_subset1_256_192', 'UPT_subset2_256_192'}
    for i, names in enumerate(want):
        raw = ds[i]
        assert raw['raw_idx'] == i
        assert sorted(raw) == sorted(['image', 'parsing', 'keypoints', 'upper_image', 'upper_parsing', 'upper_keypoints', 'lower_image',
                                      'lower_parsing', 'lower_keypoints', 'person_name', 'upper_name', 'lower_name', 'raw_idx'])
        for role, prefix, name in zip(('person', 'upper', 'lower'), ('', 'upper_', 'lower_'), names):
            assert raw[role + '_name'] == _path(name), (i, role)
            image, parsing, kp = by_name[_path(name)]                # resolved exactly as the pair lists' names are
            assert raw[prefix + 'image'].dtype == np.uint8 and raw[prefix + 'image'].shape == (256, 192, 3)
            assert np.array_equal(raw[prefix + 'image'], image) and np.array_equal(raw[prefix + 'parsing'], parsing)
            assert raw[prefix + 'keypoints'].dtype == np.float64 and np.array_equal(raw[prefix + 'keypoints'], kp)
    # the files a name resolves to
    image, parsing, keypoints = ds._outfits[0][1]
    ds0, f0 = c0.split('/')
    assert (image, parsing, keypoints) == (os.path.join(ds0, 'image', f0), os.path.join(ds0, 'parsing', f0[:-4] + '_label.png'),
                                           os.path.join(ds0, 'keypoints', f0[:-4] + '_keypoints.json'))
    # '-' is the person's own arrays, and a file named twice on a line is decoded once
    own = ds[2]
    assert own['upper_image'] is own['image'] and own['lower_parsing'] is own['parsing'] and own['upper_keypoints'] is own['keypoints']
    assert own['upper_name'] == own['lower_name'] == own['person_name']
    ds2, _ = _dataset(tree, tmp_path, '%s %s %s\n' % (p0, c0, c0))
    twice = ds2[0]
    assert twice['upper_image'] is twice['lower_image'] and twice['upper_image'] is not twice['image']


def test_every_refusal_names_the_file_and_the_line(tree, tmp_path):
    p0, c0 = _name(0, 'p'), _name(0, 'c')
    good = '%s %s %s\n' % (p0, c0, c0)
    cases = [(good + '\n' + '%s %s\n' % (p0, c0), 3, 'fields'),                      # two fields, after a blank line: line 3
             (good + '%s %s %s %s\n' % (p0, c0, c0, c0), 2, 'fields'),               # four fields
             ('%s\n' % p0, 1, 'fields'),
             (good + good + '%s Zalando_512_320/c0.jpg %s\n' % (p0, c0), 3, 'sub-dataset'),      # a sub-dataset of the 512 tree
             (good + '%s MPV_256_192/c0.jpg %s\n' % (p0, c0), 2, 'sub-dataset'),     # a training sub-dataset, not a test one
             (good + '%s %s p9.jpg\n' % (p0, c0), 2, 'sub-dataset'),                 # no sub-dataset at all
             ('\n\n- %s %s\n' % (c0, c0), 3, 'person')]
    for text, line, word in cases:
        with pytest.raises(ValueError) as e:
            _dataset(tree, tmp_path, text)
        message = str(e.value)
        assert str(tmp_path / 'outfits.txt') in message and 'line %d' % line in message and word in message, (text, message)
    with pytest.raises(IOError):
        _dataset(tree, tmp_path, '\n\n')                             # no outfit at all
    ds, _ = _dataset(tree, tmp_path, good + '%s UPT_subset2_256_192/nobody.jpg -\n' % p0)
    assert len(ds) == 2 and ds[0]['raw_idx'] == 0
    with pytest.raises(IOError):                                     # a missing file: at load, as the pairs' data set
        ds[1]
    with pytest.raises(IOError):
        _dataset(str(tmp_path / 'missing'), tmp_path, good)
    with pytest.raises(IOError, match='resolution'):
        _dataset(tree, tmp_path, good, resolution=512)


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
    assert b['people_image'].dtype == torch.uint8 and tuple(b['people_image'].shape) == (4, 256, 192, 3)
    assert b['people_parsing'].dtype == torch.uint8 and tuple(b['people_parsing'].shape) == (4, 256, 192)
    assert b['people_keypoints'].dtype == torch.float64 and tuple(b['people_keypoints'].shape) == (4, 18, 3)
    for role, prefix in (('person', ''), ('upper', 'upper_'), ('lower', 'lower_')):
        assert b[role + '_name'] == [s[role + '_name'] for s in samples]
        for i, s in enumerate(samples):
            j = int(b[role + '_idx'][i])
            assert b['people_name'][j] == s[role + '_name'] and np.array_equal(b['people_image'][j].numpy(), s[prefix + 'image'])
            assert np.array_equal(b['people_parsing'][j].numpy(), s[prefix + 'parsing'])
            assert np.array_equal(b['people_keypoints'][j].numpy(), s[prefix + 'keypoints'])
    one = collate_outfits(samples[1:2])                              # a batch that is one '- -' line: one person
    assert one['people_name'] == [_path(p0)] and one['person_idx'].tolist() == one['upper_idx'].tolist() == one['lower_idx'].tolist() == [0]


def test_a_pair_is_the_outfit_of_its_change_region(tree):
    import functools
    from training.dataset import UvitonDatasetV19_test, collate_region_outfits, pair_as_outfit
    pairs = UvitonDatasetV19_test(path=tree)
    raw = pairs[1]
    whose = dict(upperbody=('clothes_', ''), lowerbody=('', 'clothes_'), fullbody=('clothes_', 'clothes_'))
    for region, (upper, lower) in whose.items():
        o = pair_as_outfit(raw, region)
        assert o['image'] is raw['image'] and o['person_name'] == raw['person_name'] and o['raw_idx'] == 1
        for prefix, src in (('upper_', upper), ('lower_', lower)):
            for k in ('image', 'parsing', 'keypoints'):
                assert o[prefix + k] is raw[src + k], (region, prefix, k)
            assert o[prefix + 'name'] == raw[(src or 'person_') + 'name'], (region, prefix)
    with pytest.raises(ValueError, match='change region'):
        pair_as_outfit(raw, 'legs')
    b = functools.partial(collate_region_outfits, 'lowerbody')([pairs[0], pairs[1]])
    assert b['clothes_name'] == [pairs[i]['clothes_name'] for i in (0, 1)] and b['upper_name'] == b['person_name']
    assert b['lower_name'] == b['clothes_name'] and len(b['people_name']) == 4 and b['upper_idx'].tolist() == b['person_idx'].tolist()


def test_a_collated_pair_batch_is_the_outfit_batch_of_its_region(tree):
    """``pairs_batch_as_outfits``, what the pair builders put in front of the outfit builders: the persons, then the donors,
    nobody looked up twice.  Pair 1 comes twice, so its two people are in the stack twice, where ``collate_region_outfits``
    of the same samples stacks them once; through the indices both name the same arrays."""
    from training.dataset import (UvitonDatasetV19_test, collate_outfits, collate_pairs, collate_region_outfits, pair_as_outfit,
                                  pairs_batch_as_outfits)
    pairs = UvitonDatasetV19_test(path=tree)
    samples = [pairs[1], pairs[0], pairs[1]]
    n = len(samples)
    raw = collate_pairs(samples)
    person, donor = list(range(n)), list(range(n, 2 * n))
    whose = dict(upperbody=(donor, person), lowerbody=(person, donor), fullbody=(donor, donor))
    for region, (upper, lower) in whose.items():
        b = pairs_batch_as_outfits(raw, region)
        dedup = collate_region_outfits(region, samples)
        assert sorted(b) == sorted(dedup) == sorted(list(collate_outfits([pair_as_outfit(s, region) for s in samples])) + ['clothes_name'])
        assert b['people_name'] == raw['person_name'] + raw['clothes_name'] and len(dedup['people_name']) == 4 < len(b['people_name']) == 2 * n
        assert b['person_idx'].tolist() == person and b['upper_idx'].tolist() == upper and b['lower_idx'].tolist() == lower
        assert b['person_name'] == raw['person_name'] and b['clothes_name'] == raw['clothes_name'] and b['raw_idx'].tolist() == [1, 0, 1]
        assert b['upper_name'] == dedup['upper_name'] and b['lower_name'] == dedup['lower_name']
        for k, dtype, shape in (('people_image', torch.uint8, (2 * n, 256, 192, 3)), ('people_parsing', torch.uint8, (2 * n, 256, 192)),
                                ('people_keypoints', torch.float64, (2 * n, 18, 3))):
            assert b[k].dtype == dtype and tuple(b[k].shape) == shape and b[k].dtype == dedup[k].dtype, k
            assert torch.equal(b[k], torch.cat([raw[k[len('people_'):]], raw['clothes_' + k[len('people_'):]]])), k
        for role in ('person', 'upper', 'lower'):
            ix, ix_dedup = b[role + '_idx'], dedup[role + '_idx']
            # what the builders assert of a batch of collate_outfits
            assert ix.dtype == torch.int64 and tuple(ix.shape) == (n,) and int(ix.min()) >= 0 and int(ix.max()) < len(b['people_image'])
            assert [b['people_name'][j] for j in ix.tolist()] == b[role + '_name'] == [dedup['people_name'][j] for j in ix_dedup.tolist()]
            for k in ('people_image', 'people_parsing', 'people_keypoints'):
                assert torch.equal(b[k][ix], dedup[k][ix_dedup]), (region, role, k)
        assert torch.equal(b['people_image'][0], b['people_image'][2]) and not torch.equal(b['people_image'][0], b['people_image'][1])
    with pytest.raises(ValueError, match='change region'):
        pairs_batch_as_outfits(raw, 'legs')


def test_the_entries_are_declared_typed_and_exported():
    from torch_utils import custom_ops
    header = open(os.path.join(ROOT, 'include', 'pasta_hip.h')).read()
    lib = custom_ops.get_plugin()
    # the label masks with six_is_lower, the eroded composite with radius and radii
    for name, args in (('pasta_tryon_outfit_masks_u8', 17), ('pasta_patch_composite_eroded_u8', 15)):
        assert re.search(r'\bint %s\(' % name, header) and hasattr(lib, name), name
        assert name in custom_ops.ABI and len(custom_ops.ABI[name][1]) == args
    assert lib.pasta_abi_version() == custom_ops.EXPECTED_ABI == 22


def test_cli_lists_the_options_and_refuses_outfits_with_a_region(tmp_path):
    run = lambda *args: subprocess.run([sys.executable, CLI, *args], capture_output=True, text=True, timeout=120, cwd=ROOT)
    r = run('--help')
    assert r.returncode == 0 and '--outfits' in r.stdout and '--change-region' in r.stdout and '--scores' in r.stdout, r.stderr
    assert 'upperbody' in r.stdout and 'lowerbody' in r.stdout and 'fullbody' in r.stdout
    # nothing of this exists: the refusal comes before any file is read, the snapshot included
    r = run('--network', str(tmp_path / 'none.pkl'), '--outdir', str(tmp_path / 'out'), '--dataroot', str(tmp_path / 'nowhere'), '--outfits',
            str(tmp_path / 'outfits.txt'), '--change-region', 'upperbody')
    assert r.returncode == 2 and '--outfits' in r.stderr and '--change-region' in r.stderr and 'exclude' in r.stderr, (r.returncode, r.stderr)
    assert 'none.pkl' not in r.stderr and not (tmp_path / 'out').exists()
    r = run('--network', str(tmp_path / 'none.pkl'), '--outdir', str(tmp_path / 'out'), '--dataroot', str(tmp_path), '--change-region', 'legs')
    assert r.returncode == 2 and 'legs' in r.stderr
