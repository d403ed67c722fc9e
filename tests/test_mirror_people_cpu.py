"""Mirrored people without a GPU (--mirror-people; include/pasta_hip.h, pasta_tryon_mirror_u8): the tables of
training/tryon_batch.py against the numpy statement (tests/mirror_ref.py), that the exchange of left and right is the right one
(the unchanged palm rule of tests/tryon_ref.py on mirrored raw samples), the data set's doubled index, the command line and the
data-set options the scores use."""
import json
import os

import numpy as np
import pytest
import torch
from click.testing import CliRunner

import mirror_ref as MR
import tryon_ref as R
import tryon_tree
from train_grid_tree import make_tree as make_cli_tree
from tryon_512_train_tree import make_512_train_tree

H, W = 256, 192

# ---- tables ----

def test_lut_is_an_involution_that_moves_the_six_labels():
    from training.tryon_batch import MIRROR_LABELS, mirror_lut
    lut = mirror_lut()
    assert lut.dtype == np.uint8 and lut.shape == (256,) and np.array_equal(lut, MR.lut())
    assert np.array_equal(lut[lut], np.arange(256))
    assert sorted(np.flatnonzero(lut != np.arange(256))) == [14, 15, 16, 17, 18, 19]
    assert [int(lut[v]) for v in (14, 15, 16, 17, 18, 19)] == [15, 14, 17, 16, 19, 18]
    assert sorted(MIRROR_LABELS) == sorted(MR.LABEL_PAIRS)


def test_mirror_keypoints_equals_the_statement_and_is_an_involution():
    from training.tryon_batch import MIRROR_JOINTS, mirror_keypoints
    assert sorted(MIRROR_JOINTS) == sorted(MR.JOINT_PAIRS)
    rng = np.random.default_rng(0)
    kp = np.zeros([4, 18, 3])
    kp[..., 0] = rng.integers(-30 * 8, 230 * 8, [4, 18]) / 8          # multiples of 1/8, also outside the canvas
    kp[..., 1] = rng.integers(-30 * 8, 290 * 8, [4, 18]) / 8
    kp[..., 2] = rng.uniform(0, 1, [4, 18])
    kp[1, 3, 2] = 0.0                                                  # a joint without confidence is reflected all the same
    kp[2] = 0.0                                                        # an empty ``people``
    for width in (192, 320):
        flags = np.array([1, 1, 1, 0], np.uint8)
        got = mirror_keypoints(kp, width, flags)
        assert got.dtype == np.float64 and got is not kp
        for i in range(3):
            assert np.array_equal(got[i], MR.mirror_keypoints(kp[i], width)), i
        assert got[3].tobytes() == kp[3].tobytes()
        assert np.array_equal(got[1, 6], [(width - 1) - kp[1, 3, 0], kp[1, 3, 1], 0.0])
        assert np.array_equal(got[2, :, 0], np.full(18, width - 1.0)) and not got[2, :, 1:].any()
        assert mirror_keypoints(got, width, flags).tobytes() == kp.tobytes()
    plain = rng.uniform(-50, 300, [3, 18, 3])
    assert mirror_keypoints(plain, 192, np.zeros(3, np.uint8)).tobytes() == plain.tobytes()
    assert mirror_keypoints(torch.from_numpy(plain), 192, torch.zeros(3, dtype=torch.uint8)).tobytes() == plain.tobytes()


# ---- the exchange is the right one: the palm rule on mirrored raw samples, no kernel involved ----

def _arms_person(seed, right_arm=True):
    """The base pose of tests/tryon_tree.py with its jitter rounded to 1/8 and confidence 0.9; discs of radius 20 of label 14
    around the left arm's joints and, with ``right_arm``, of label 15 around the right arm's."""
    rng = np.random.default_rng(seed)
    kp = tryon_tree.person_keypoints(0, rng)
    kp[:, :2] = np.round(kp[:, :2] * 8) / 8
    kp[:, 2] = 0.9
    parsing = np.zeros([H, W], np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    sides = ((14, (5, 6, 7)), (15, (2, 3, 4))) if right_arm else ((14, (5, 6, 7)),)
    for label, joints in sides:
        for j in joints:
            parsing[(yy - kp[j, 1]) ** 2 + (xx - kp[j, 0]) ** 2 < 20 ** 2] = label
    if not right_arm:
        kp[[2, 3, 4], 2] = 0.0
    image = rng.integers(0, 256, [H, W, 3], dtype=np.uint8)
    return dict(image=image, parsing=parsing, keypoints=kp, raw_idx=0)


def _palm(sample):
    return R.label_masks(sample['image'], sample['parsing'], sample['keypoints'])[8]


def _without_label_exchange(sample):
    wrong = MR.mirror_raw(sample)
    wrong['parsing'] = np.ascontiguousarray(sample['parsing'][:, ::-1])
    return wrong


def _box(mask, r, op):
    """The maximum (dilation) or minimum (erosion) over the (2r + 1)^2 box, the outside counting as 0."""
    h, w = mask.shape
    pad = np.zeros([h + 2 * r, w + 2 * r], mask.dtype)
    pad[r:r + h, r:r + w] = mask
    return op([pad[dy:dy + h, dx:dx + w] for dy in range(2 * r + 1) for dx in range(2 * r + 1)], axis=0)


# Seeds 0..6 without 2.  Seed 2's pose puts the leftmost column of the right elbow's disc exactly on the edge of the dilated
# forearm box: the 16 x 16 box covers offsets -8..7, so mirrored it ends one column earlier and leaves that column (11 pixels) in
# the palm, a sliver of its own 30 pixels from the rest of the palm.  That is the rule's stated asymmetry, not a wrong
# exchange, and "near the ORIGINAL palm's boundary" cannot hold for a component the original does not have; the test below states
# what holds there.
@pytest.mark.parametrize('seed', [0, 1, 3, 4, 5, 6])
def test_mirrored_palm_is_the_flipped_palm_up_to_its_boundary(seed):
    sample = _arms_person(seed)
    palm = _palm(sample)
    back = _palm(MR.mirror_raw(sample))[:, ::-1]         # the padding is symmetric (32 columns on either side)
    count, mirrored = int(palm.sum()), int(back.sum())
    boundary = palm & (1 - _box(palm, 1, np.min))        # palm pixels with a neighbour outside the palm
    differ = palm != back
    far = differ & (_box(boundary, 2, np.max) == 0)
    print('seed %d: palm %d pixels, mirrored %d (%.2f %%), %d differ, %d farther than 2 from the boundary'
          % (seed, count, mirrored, 100.0 * abs(mirrored - count) / count, int(differ.sum()), int(far.sum())))
    assert count > 100
    assert abs(mirrored - count) <= 0.05 * count
    assert not far.any()
    # what a flip without the label exchange would give: the hands paired with the other side's arm, hardly anything removed
    wrong = int(_palm(_without_label_exchange(sample)).sum())
    print('         without the label exchange: %d pixels (%.1f times)' % (wrong, wrong / count))
    assert wrong > 2 * count


def test_a_sliver_at_the_edge_of_a_hand_is_the_box_asymmetry():
    """Seed 2 (see above): the count still agrees within 5 %, and a differing pixel is within 2 of the original palm's boundary or
    is itself a boundary pixel of the hand labels, where a box edge one column off shows."""
    sample = _arms_person(2)
    palm = _palm(sample)
    back = _palm(MR.mirror_raw(sample))[:, ::-1]
    assert abs(int(back.sum()) - int(palm.sum())) <= 0.05 * int(palm.sum())
    hand = np.pad(np.isin(sample['parsing'], (14, 15)).astype(np.uint8), ((0, 0), (32, 32)))
    hand_edge = hand & (1 - _box(hand, 1, np.min))
    boundary = palm & (1 - _box(palm, 1, np.min))
    differ = palm != back
    far = differ & (_box(boundary, 2, np.max) == 0)
    print('seed 2: %d differ, %d of them away from the palm, %d of those on the edge of a hand' % (differ.sum(), far.sum(), (far & (hand_edge == 1)).sum()))
    assert far.any() and not (far & (hand_edge == 0)).any()
    assert int(_palm(_without_label_exchange(sample)).sum()) > 2 * int(palm.sum())


@pytest.mark.parametrize('seed', range(6))
def test_one_armed_person_keeps_the_palm(seed):
    sample = _arms_person(seed, right_arm=False)
    assert _palm(sample).any()
    assert _palm(MR.mirror_raw(sample)).any()
    assert not _palm(_without_label_exchange(sample)).any()


# ---- the data set ----

@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return tryon_tree.make_tree(tmp_path_factory.mktemp('mirror_cpu'))


@pytest.fixture(scope='module')
def tree_512(tmp_path_factory):
    return make_512_train_tree(tmp_path_factory.mktemp('mirror_cpu_512'))


def _same_files(a, b):
    return all(np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in ('image', 'parsing', 'keypoints', 'erase_mask'))


def test_dataset_doubles_with_flags(tree):
    from training.dataset import UvitonDatasetFull, collate
    plain, ds = UvitonDatasetFull(tree), UvitonDatasetFull(tree, mirror_people=True)
    assert len(plain) == 5 and len(ds) == 10
    samples = [ds[i] for i in range(10)]
    assert [s['xflip'] for s in samples] == [0] * 5 + [1] * 5
    assert [s['raw_idx'] for s in samples] == [0, 1, 2, 3, 4] * 2
    for i in range(5):
        assert _same_files(samples[i], samples[5 + i]) and _same_files(samples[i], plain[i]), i      # the files as they are
    assert ds.vis_index == plain.vis_index and _same_files(ds.load_raw(3), plain.load_raw(3)) and 'xflip' not in ds.load_raw(3)
    assert ds.image_shape == plain.image_shape and ds.resolution == 256
    assert all(ds[i]['xflip'] == 0 for i in ds.vis_index)          # the sample grid reads unmirrored people
    assert len(UvitonDatasetFull(tree, mirror_people=True, max_size=3)) == 6
    sub = UvitonDatasetFull(tree, mirror_people=True, max_size=3, random_seed=1)
    assert [sub[i]['raw_idx'] for i in range(3)] == [sub[i]['raw_idx'] for i in range(3, 6)]
    assert [sub[i]['xflip'] for i in range(6)] == [0, 0, 0, 1, 1, 1]
    batch = collate([samples[1], samples[7], samples[9]])
    assert batch['xflip'].dtype == torch.uint8 and batch['xflip'].tolist() == [0, 1, 1] and batch['raw_idx'].tolist() == [1, 2, 4]


def test_dataset_without_the_option_is_what_it_was(tree):
    from training.dataset import UvitonDatasetFull, collate
    for ds in (UvitonDatasetFull(tree), UvitonDatasetFull(tree, mirror_people=False)):
        assert len(ds) == 5
        assert sorted(ds[0]) == ['erase_mask', 'image', 'keypoints', 'parsing', 'raw_idx']
        assert sorted(collate([ds[0], ds[1]])) == ['erase_hw', 'erase_masks', 'image', 'keypoints', 'parsing', 'raw_idx']
    with pytest.raises(ValueError, match='xflip'):
        UvitonDatasetFull(tree, xflip=True)
    with pytest.raises(ValueError, match='xflip'):
        UvitonDatasetFull(tree, xflip=True, mirror_people=True)


def test_dataset_512_doubles_with_flags(tree_512):
    from training.dataset import UvitonDatasetFull_512
    plain, ds = UvitonDatasetFull_512(tree_512), UvitonDatasetFull_512(tree_512, mirror_people=True)
    assert len(plain) == 5 and len(ds) == 10 and ds.vis_index == plain.vis_index
    assert [ds[i]['xflip'] for i in range(10)] == [0] * 5 + [1] * 5
    assert [ds[i]['raw_idx'] for i in range(10)] == [0, 1, 2, 3, 4] * 2
    assert _same_files(ds[1], ds[6]) and 'xflip' not in plain[1]
    assert len(UvitonDatasetFull_512(tree_512, mirror_people=True, max_size=3)) == 6


def test_builders_take_a_batch_without_flags_as_it_is():
    """``mirror_batch`` decides on the host from the batch alone: no key or no flag set returns its arguments, untouched."""
    from training.tryon_batch import mirror_batch
    image, parsing, erase = torch.zeros([2, 4, 3, 3], dtype=torch.uint8), torch.zeros([2, 4, 3], dtype=torch.uint8), torch.zeros([2, 2, 2], dtype=torch.uint8)
    kp, hw = np.zeros([2, 18, 3]), torch.ones([2, 2], dtype=torch.int32)
    for raw in ({}, dict(xflip=torch.zeros(2, dtype=torch.uint8))):
        got = mirror_batch(raw, image, parsing, kp, erase, hw)
        assert got[0] is image and got[1] is parsing and got[2] is kp and got[3] is erase


# ---- the command line ----

@pytest.fixture(scope='module')
def cli_tree(tmp_path_factory):
    return make_cli_tree(tmp_path_factory.mktemp('mirror_cli'))


def _options(output):
    text = output[output.index('Training options:') + len('Training options:'):output.index('Output directory:')]
    return json.loads(text)


def _run(tree, outdir, *extra):
    import train_wo_flow_fullbody as T
    return CliRunner().invoke(T.main, ['--outdir', str(outdir), '--data', tree, '--dry-run', *extra])


def test_mirror_people_option(cli_tree, tmp_path):
    from training.dataset import UvitonDatasetFull
    people = len(UvitonDatasetFull(cli_tree))
    plain = _run(cli_tree, tmp_path / 'runs', '--cfg', 'fashion', '--subset', str(people))
    on = _run(cli_tree, tmp_path / 'runs', '--cfg', 'fashion', '--subset', str(people), '--mirror-people', 'true')
    off = _run(cli_tree, tmp_path / 'runs', '--cfg', 'fashion', '--subset', str(people), '--mirror-people', 'false')
    assert plain.exit_code == 0 and on.exit_code == 0 and off.exit_code == 0, (plain.output, on.output, off.output)
    assert off.output == plain.output
    a, b = _options(plain.output), _options(on.output)
    assert not a['training_set_kwargs'].get('mirror_people', False) and '-mirrorpeople' not in plain.output
    assert b['training_set_kwargs'].pop('mirror_people') is True
    assert b['training_set_kwargs']['max_size'] == people                     # the unmirrored count
    assert b.pop('run_dir') == a.pop('run_dir').replace('-subset%d' % people, '-subset%d-mirrorpeople' % people)
    a['training_set_kwargs'].pop('mirror_people', None)
    assert b == a
    assert 'Number of images:   %d' % people in on.output and 'Mirrored people:    True' in on.output and 'Mirrored people:    False' in plain.output
    assert len(UvitonDatasetFull(**{k: v for k, v in _options(on.output)['training_set_kwargs'].items() if k != 'class_name'})) == 2 * people
    # the reference's --mirror stays refused, and says where to go
    res = _run(cli_tree, tmp_path / 'runs', '--mirror', 'true')
    assert res.exit_code != 0 and 'mirrored key points' in res.output and '--mirror-people' in res.output


def test_continue_counts_the_people_unmirrored(cli_tree, tmp_path):
    """A state file written by train_state's helper with the options of a mirrored dry run: --continue accepts it (the recorded
    max_size is N people, the mirrored set holds 2N), keeps the option and refuses to change it."""
    from training import train_state
    res = _run(cli_tree, tmp_path / 'runs', '--cfg', 'fashion', '--batch', '2', '--kimg', '5', '--mirror-people', 'true')
    assert res.exit_code == 0, res.output
    options = _options(res.output)
    run_dir = tmp_path / 'runs' / os.path.basename(options['run_dir'])
    os.makedirs(run_dir)
    empty = dict(cur_nimg=0, batch_idx=0, cur_tick=1, elapsed_sec=0.0, num_gpus=1, batch_size=2, batch_gpu=2, random_seed=0,
                 options=json.dumps(options, indent=2), G={}, D={}, G_ema={}, opt={}, grid_z=torch.zeros([0, 0]), ranks=[])
    train_state.save_state(str(run_dir / 'training-state-000000.pt'), None, empty)
    res = _run(cli_tree, tmp_path / 'out', '--continue', str(run_dir))
    assert res.exit_code == 0, res.output
    got = _options(res.output)
    assert got['training_set_kwargs']['mirror_people'] is True and got['training_set_kwargs']['max_size'] == options['training_set_kwargs']['max_size']
    name = os.path.basename(got['run_dir'])
    assert '-mirrorpeople-fashion-' in name and name.endswith('-continue000000')
    for value in ('true', 'false'):
        res = _run(cli_tree, tmp_path / 'out', '--continue', str(run_dir), '--mirror-people', value)
        assert res.exit_code != 0 and '--mirror-people cannot be given with --continue' in res.output, res.output


# ---- scoring never sees mirrored people ----

@pytest.mark.parametrize('metric', ['recon_full', 'recon2k'])
def test_scores_force_the_option_off(monkeypatch, metric):
    from metrics import metric_main, reconstruction
    seen = {}
    def compute(opts, name):
        seen.update(opts.dataset_kwargs)
        return {name + '_l1': 0.0}
    monkeypatch.setattr(reconstruction, 'compute', compute)
    kwargs = dict(class_name='training.dataset.UvitonDatasetFull', path='x', use_labels=False, max_size=5, xflip=False, mirror_people=True)
    metric_main.calc_metric(metric, G=None, dataset_kwargs=kwargs, num_gpus=1, rank=0, device=torch.device('cpu'))
    assert seen['mirror_people'] is False and seen['xflip'] is False and seen['path'] == 'x'
    assert kwargs['mirror_people'] is True              # the caller's dictionary is not touched
