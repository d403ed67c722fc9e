"""Training at 512 x 320 without a GPU: the data set (training.dataset.UvitonDatasetFull_512), how the commands pick it from
the tree, the numpy restatement (tests/tryon_512_train_ref.py) on hand-made cases, the condition on the fixtures that keeps
both branches of the erase rule under test, and the two new entries in the C interface."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
from click.testing import CliRunner

import tryon_512_train_ref as TR
from conftest import ROOT
from tryon_512_train_tree import ERASE_SIZES, PERSONS, VIS_INDEX, make_512_train_tree


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return make_512_train_tree(tmp_path_factory.mktemp('train512_cpu'))


def test_dataset_lists_the_tree_in_order(tree):
    from training.dataset import UvitonDatasetFull, UvitonDatasetFull_512, collate
    ds = UvitonDatasetFull_512(tree)
    assert isinstance(ds, UvitonDatasetFull) and len(ds) == len(PERSONS)
    assert ds._image_fnames == [os.path.join(d, 'image', e) for d, e in PERSONS]
    assert ds._parsing_fnames == [os.path.join(d, 'parsing', e.replace('.jpg', '_label.png')) for d, e in PERSONS]     # MPV too
    assert ds._kpt_fnames == [os.path.join(d, 'keypoints', e.replace('.jpg', '_keypoints.json')) for d, e in PERSONS]
    assert ds.vis_index == VIS_INDEX                   # nowhere.jpg is skipped, p2 is found under Deepfashion's image/train
    assert ds.resolution == 512 and ds.image_shape == [3, 512, 512]
    count = len(os.listdir(os.path.join(tree, 'train_random_mask_acgpn')))
    assert count == len(ERASE_SIZES)
    for i in range(len(ds)):
        s = ds[i]
        assert sorted(s) == ['erase_mask', 'image', 'keypoints', 'parsing', 'raw_idx']
        assert s['image'].shape == (512, 320, 3) and s['image'].dtype == np.uint8 and s['parsing'].shape == (512, 320)
        assert s['keypoints'].shape == (18, 3) and s['keypoints'].dtype == np.float64 and s['raw_idx'] == i
        assert s['erase_mask'].ndim == 2 and s['erase_mask'].shape in ERASE_SIZES
        assert s['erase_mask'].shape == ds[i % count]['erase_mask'].shape       # file raw_idx % count
    assert ds[1]['keypoints'][7, 2] == 0.05 and ds[3]['keypoints'][3, 0] == -110.5     # unshifted, as written
    batch = collate([ds[i] for i in range(len(ds))])
    assert tuple(batch['image'].shape) == (5, 512, 320, 3) and tuple(batch['keypoints'].shape) == (5, 18, 3)
    assert tuple(batch['erase_masks'].shape) == (5, 512, 512) and sorted(map(tuple, batch['erase_hw'].tolist())) == sorted(
        [ds[i]['erase_mask'].shape for i in range(5)])
    with pytest.raises(IOError, match='resolution'):
        UvitonDatasetFull_512(tree, resolution=256)


def test_builder_for_picks_by_class(tree):
    from training.dataset import UvitonDatasetFull_512, UvitonDatasetFull_512_test
    from training.tryon_batch import FullBodyBatchBuilder, builder_for
    from training.tryon_regions import FullBodyRegionBatchBuilder
    b = builder_for(UvitonDatasetFull_512(tree), 'cpu')
    assert type(b) is FullBodyRegionBatchBuilder
    assert (b.lower_parts, b.x_pad, b.shin_fallback, b.shifted) == ((0, 6, 7, 8, 9), 0, False, True)
    a = FullBodyBatchBuilder('cpu')
    assert (a.lower_parts, a.x_pad, a.shin_fallback, a.shifted) == ((6, 7, 8, 9), 32, False, False)
    with pytest.raises(TypeError):
        builder_for(object(), 'cpu')


def _dry_run(tree, outdir, *extra):
    import train_wo_flow_fullbody as T
    return CliRunner().invoke(T.main, ['--outdir', str(outdir), '--data', tree, '--dry-run', *extra])


def _options(output):
    return json.loads(output[output.index('Training options:') + len('Training options:'):output.index('Output directory:')])


def test_dry_run_on_the_512_tree(tree, tmp_path):
    res = _dry_run(tree, tmp_path / 'runs')
    assert res.exit_code == 0, res.output
    o = _options(res.output)
    assert o['training_set_kwargs']['class_name'] == 'training.dataset.UvitonDatasetFull_512'
    assert o['training_set_kwargs']['resolution'] == 512 and o['training_set_kwargs']['max_size'] == len(PERSONS)
    cfg = o['cfg']
    assert cfg['G_kwargs']['patch_channels'] == 45 and cfg['G_kwargs']['img_resolution'] == cfg['D_kwargs']['img_resolution'] == 512
    # --cfg auto at 512 on one GPU: mb = 8, fmaps = 1, gamma = 0.0002 * 512^2 / 8
    assert o['batch_size'] == 8 and cfg['G_kwargs']['synthesis_kwargs']['channel_base'] == 32768
    assert cfg['loss_kwargs']['r1_gamma'] == 0.0002 * 512 ** 2 / 8
    assert re.search(r'Data set class: +UvitonDatasetFull_512\n', res.output) and re.search(r'Image resolution: +512\n', res.output)
    assert not (tmp_path / 'runs').exists()


def test_metrics_data_follows_the_same_choice(tree, tmp_path):
    from train_grid_tree import make_tree
    res = _dry_run(tree, tmp_path / 'runs', '--metrics', 'recon_full', '--metrics_data', tree)
    assert res.exit_code == 0, res.output
    assert _options(res.output)['metric_set_kwargs']['class_name'] == 'training.dataset.UvitonDatasetFull_512'
    tree256 = make_tree(tmp_path / 'tree256')
    res = _dry_run(tree, tmp_path / 'runs', '--metrics', 'recon_full', '--metrics_data', tree256)
    assert res.exit_code != 0 and 'resolution 256, the training data has 512' in res.output, res.output


def test_a_tree_with_both_layouts_trains_as_256(tmp_path):
    from train_grid_tree import make_tree
    from training.dataset import training_set_class
    tree256 = make_tree(tmp_path / 'both')
    os.makedirs(os.path.join(tree256, 'Zalando_512_320', 'image'))
    assert training_set_class(tree256) == 'training.dataset.UvitonDatasetFull'
    res = _dry_run(tree256, tmp_path / 'runs')
    assert res.exit_code == 0, res.output
    o = _options(res.output)
    assert o['training_set_kwargs']['class_name'] == 'training.dataset.UvitonDatasetFull' and o['training_set_kwargs']['resolution'] == 256
    assert 'patch_channels' not in o['cfg']['G_kwargs']
    # neither layout: the error names the 256 one, as before
    res = _dry_run(str(tmp_path), tmp_path / 'runs')
    assert res.exit_code != 0 and '--data:' in res.output and 'Zalando_256_192' in res.output


# ---- the restatement on hand-made cases ----

def test_gt_parsing_labels():
    lab = np.arange(20, dtype=np.uint8).reshape(4, 5)
    want = np.zeros(20, np.uint8)
    for label, cls in ((5, 1), (6, 1), (7, 1), (9, 2), (12, 2), (14, 3), (15, 3), (16, 4), (17, 4), (10, 5)):
        want[label] = cls
    assert np.array_equal(TR.gt_parsing(lab), want.reshape(4, 5))


def test_erase_rule_wraps_in_uint8():
    side = 8
    arm = np.zeros([4, side, side], np.uint8)
    arm[0] = arm[1] = 1                                # arm masks 0 and 1 do not take part
    arm[2, 2:6, 2:6] = 1
    arm[3, 4:8, 4:8] = 1
    mask = np.zeros([side, side], np.uint8)            # the size of the square: the resize is the identity
    assert np.array_equal(TR.erase_mask(arm, mask, side), ((arm[2] + arm[3]) > 0).astype(np.uint8))     # only the arm masks erase
    mask[4, 4], mask[5, 5], mask[0, 0], mask[2, 2], mask[7, 7] = 254, 255, 3, 255, 254
    erase = TR.erase_mask(arm, mask, side)
    assert erase[4, 4] == 0                            # 1 + 1 + 254 wraps to 0: NOT erased
    assert erase[5, 5] == 1 and erase[0, 0] == 1       # 257 -> 1; a mask value of 3 alone erases
    assert erase[2, 2] == 0 and erase[7, 7] == 1       # 1 + 255 wraps; 1 + 254 = 255 does not
    assert erase[1, 1] == 0 and erase[3, 3] == 1


@pytest.fixture(scope='module')
def cases(tree):
    return TR.cases(tree)


def test_fixtures_exercise_both_branches_of_the_erase(cases):
    """On the numpy reference alone: on every sample between 5 % and 60 % of the non-zero pixels of denorm_upper are erased, so
    neither branch of the erase can go untested; the three mask sizes are present and the wrap pixel is kept."""
    samples, stages, wrap = cases
    assert [s['erase_mask'].shape for s in samples] == list(ERASE_SIZES)
    for i, (s, st) in enumerate(zip(samples, stages)):
        erase, du, dl = TR.erased(st, s['erase_mask'])
        lit = st['denorm_upper'].any(axis=2)
        share = float(erase[lit].mean())
        print('sample %d: %d lit pixels of denorm_upper, %.1f %% erased' % (i, int(lit.sum()), 100 * share))
        assert 0.05 <= share <= 0.60, (i, share)
        assert st['denorm_lower'].any() and st['palm'].any() and set(np.unique(st['gt_parsing'])) == {0, 1, 2, 3, 4, 5}
    a = stages[0]['arm_masks']
    assert a[2][wrap] == 1 and a[3][wrap] == 1 and samples[0]['erase_mask'][wrap] == 254
    erase, du, _ = TR.erased(stages[0], samples[0]['erase_mask'])
    assert erase[wrap] == 0 and du[wrap].any()
    around = erase[wrap[0] - 1:wrap[0] + 2, wrap[1] - 1:wrap[1] + 2]
    assert around.sum() >= 4                           # its neighbours under the arm masks are erased
    # person 1: no left wrist (part 3) and no right ankle (part 9), and no shin fall-back; person 2's arm reaches off the square
    valid = [[bool(st['M_invs'][k].any()) for k in range(10)] for st in stages]
    assert all(valid[0]) and valid[1] == [True, True, True, False, True, True, True, True, True, False] and all(valid[2])
    assert not stages[1]['arm_masks'][1].any() and stages[1]['arm_masks'][2].any()


def test_interface_carries_the_two_entries():
    from torch_utils import custom_ops
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'pasta_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(pasta_[a-z0-9_]+)\s*\(', text))
    lib = ctypes.CDLL(custom_ops.build())
    for name in ('pasta_tryon_masks_u8', 'pasta_tryon_train_region_assemble'):          # the label masks are the 256 training set's entry
        assert name in declared and name in custom_ops.ABI and hasattr(lib, name), name
    assert custom_ops.EXPECTED_ABI == 22
    # bad arguments are refused on the host, before any launch
    typed = custom_ops.get_plugin()
    outs = (ctypes.c_void_p * 9)(*[1] * 9)
    assert typed.pasta_tryon_train_region_assemble(*[1] * 9, 4, 5, 1, 1, outs, 1, 512, 320, 10, 5, 128, 126, 8, 8, None) != 0
    assert b'pw a multiple of 4' in typed.pasta_last_error()
    assert typed.pasta_tryon_train_region_assemble(*[1] * 9, 4, 10, 1, 1, outs, 1, 512, 320, 10, 5, 128, 128, 8, 8, None) != 0
    assert b'arm parts 4, 10 of 10' in typed.pasta_last_error()
    assert typed.pasta_tryon_masks_u8(*[1] * 8, None, 1, 512, 320, None) != 0
    assert b'tryon_masks_u8: null pointer' in typed.pasta_last_error()
