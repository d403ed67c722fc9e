"""Jittered people without a GPU (--jitter-people; include/pasta_hip.h, pasta_tryon_jitter_u8): the numpy statement
(tests/jitter_ref.py) held to the cases whose answer is known without it, the host side of training/tryon_batch.py against the
statement, the draws, the positions the training loop attaches, the command line, and that the scores never see the option."""
import json
import os

import numpy as np
import pytest
import torch
from click.testing import CliRunner

import jitter_ref as JR
import tryon_tree
from train_grid_tree import make_tree as make_cli_tree

# ---- the statement on cases with a known answer ----

def _random_item(h, w, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, [h, w, 3], dtype=np.uint8), rng.integers(0, 256, [h, w], dtype=np.uint8)


@pytest.mark.parametrize('h,w', [(1, 1), (5, 7), (9, 16), (12, 5)])
def test_statement_identity_returns_the_input(h, w):
    image, parsing = _random_item(h, w, 0)
    got_i, got_p = JR.resample(image, parsing, JR.IDENTITY_AFFINE, JR.IDENTITY_COLOUR)
    assert got_i.dtype == np.uint8 and got_i.tobytes() == image.tobytes() and got_p.tobytes() == parsing.tobytes()
    assert JR.affine_q16(JR.IDENTITY_GEOMETRY, h, w) == list(JR.IDENTITY_AFFINE)
    assert JR.colour_q8(JR.IDENTITY_TONE) == list(JR.IDENTITY_COLOUR)


@pytest.mark.parametrize('tx,ty', [(1, 0), (-2, 0), (0, 3), (3, -2), (20, 20)])
def test_statement_integer_shift_is_the_clamped_index_shift(tx, ty):
    h, w = 7, 9
    image, parsing = _random_item(h, w, 1)
    affine = JR.affine_q16((1.0, 0.0, float(tx), float(ty)), h, w)
    assert affine == [65536, 0, -tx * 65536, 0, 65536, -ty * 65536]
    got_i, got_p = JR.resample(image, parsing, affine, JR.IDENTITY_COLOUR)
    ys, xs = np.clip(np.arange(h) - ty, 0, h - 1), np.clip(np.arange(w) - tx, 0, w - 1)
    assert np.array_equal(got_i, image[ys][:, xs]) and np.array_equal(got_p, parsing[ys][:, xs])


@pytest.mark.parametrize('side', [1, 2, 7, 8])
def test_statement_quarter_turn_on_a_square_is_rot90(side):
    image, parsing = _random_item(side, side, 2)
    affine = JR.affine_q16((1.0, 90.0, 0.0, 0.0), side, side)
    assert affine == [0, 65536, 0, -65536, 0, (side - 1) * 65536]
    got_i, got_p = JR.resample(image, parsing, affine, JR.IDENTITY_COLOUR)
    assert np.array_equal(got_i, np.rot90(image, -1)) and np.array_equal(got_p, np.rot90(parsing, -1))


def test_statement_half_pixel_shift_is_the_rounded_mean_of_two():
    h, w = 6, 11
    image, _ = _random_item(h, w, 3)
    got, _ = JR.resample(image, np.zeros([h, w], np.uint8), JR.affine_q16((1.0, 0.0, 0.5, 0.0), h, w), JR.IDENTITY_COLOUR)
    left = image[:, np.clip(np.arange(w) - 1, 0, w - 1)].astype(np.int32)
    assert np.array_equal(got, ((left + image.astype(np.int32) + 1) >> 1).astype(np.uint8))


def test_statement_negative_colour_matrix_is_the_complement():
    image, parsing = _random_item(5, 6, 4)
    negative = [-256, 0, 0, 255 * 256, 0, -256, 0, 255 * 256, 0, 0, -256, 255 * 256]
    got, _ = JR.resample(image, parsing, JR.IDENTITY_AFFINE, negative)
    assert np.array_equal(got, 255 - image)


# ---- the host side against the statement ----

def _geometries(rng, n):
    return np.stack([1.5 ** rng.uniform(-1, 1, n), rng.uniform(-45, 45, n), rng.uniform(-48, 48, n), rng.uniform(-64, 64, n)], axis=1)


def test_integers_equal_the_statement():
    from training.tryon_batch import jitter_affine_q16, jitter_colour_q8
    rng = np.random.default_rng(5)
    geometry = np.concatenate([_geometries(rng, 20), [JR.IDENTITY_GEOMETRY, (1.0, 90.0, 0.0, 0.0), (0.5, 0.0, 500.0, -500.0)]])
    tone = np.concatenate([np.stack([1.5 ** rng.uniform(-1, 1, 20), 1.5 ** rng.uniform(-1, 1, 20), rng.uniform(-32, 32, 20)], axis=1),
                           [JR.IDENTITY_TONE]])
    for H, W in ((256, 192), (512, 320), (7, 7)):
        got = jitter_affine_q16(geometry, H, W)
        assert got.dtype == np.int64 and got.shape == (23, 6)
        assert got.tolist() == [JR.affine_q16(tuple(g), H, W) for g in geometry.tolist()]
    got = jitter_colour_q8(tone)
    assert got.dtype == np.int32 and got.shape == (21, 12)
    assert got.tolist() == [JR.colour_q8(tuple(t)) for t in tone.tolist()]
    assert got[-1].tolist() == list(JR.IDENTITY_COLOUR)
    # saturation 0 is the luma in every channel, contrast scales about 128
    grey = np.asarray(JR.colour_q8((1.0, 0.0, 0.0))).reshape(3, 4)
    assert (grey[:, :3] == np.rint(np.array(JR.LUMA) * 256)).all() and not grey[:, 3].any()
    assert JR.colour_q8((2.0, 1.0, 3.0))[:4] == [512, 0, 0, (-128 + 3) * 256]


def test_jitter_keypoints():
    from training.tryon_batch import jitter_keypoints
    rng = np.random.default_rng(6)
    kp = rng.uniform(-30, 290, [4, 18, 3])
    kp[..., 2] = rng.uniform(0, 1, [4, 18])
    kp[0, 3, 2], kp[1, 0, 2], kp[1, 5, 2] = 0.05, 0.0, 0.1
    # the identity keeps the bits
    got = jitter_keypoints(kp, np.tile(JR.IDENTITY_GEOMETRY, (4, 1)), 256, 192)
    assert got.dtype == np.float64 and got is not kp and got.tobytes() == kp.tobytes()
    assert jitter_keypoints(torch.from_numpy(kp), np.tile(JR.IDENTITY_GEOMETRY, (4, 1)), 256, 192).tobytes() == kp.tobytes()
    # a quarter turn on a square canvas moves a joint where the pixel goes: rot90(image, -1)[y', x'] = image[y, x] with
    # (x', y') = (side - 1 - y, x)
    side = 7
    turn = np.tile((1.0, 90.0, 0.0, 0.0), (4, 1))
    pix = kp.copy()
    pix[..., 0], pix[..., 1] = rng.integers(0, side, [4, 18]), rng.integers(0, side, [4, 18])
    got = jitter_keypoints(pix, turn, side, side)
    seen = pix[..., 2] >= 0.1
    assert seen.sum() < seen.size
    assert np.allclose(got[seen][:, 0], side - 1 - pix[seen][:, 1], rtol=0, atol=1e-12)
    assert np.allclose(got[seen][:, 1], pix[seen][:, 0], rtol=0, atol=1e-12)
    image = rng.integers(0, 256, [side, side], dtype=np.uint8)
    turned = np.rot90(image, -1)
    for x, y, (gx, gy) in zip(pix[seen][:, 0], pix[seen][:, 1], np.rint(got[seen][:, :2])):
        assert turned[int(gy), int(gx)] == image[int(y), int(x)]
    assert np.array_equal(got[seen][:, 2], pix[seen][:, 2])
    # joints below 0.1 are untouched, bit for bit; 0.1 itself moves
    assert got[~seen].tobytes() == pix[~seen].tobytes() and not seen[0, 3] and not seen[1, 0] and seen[1, 5]
    # general parameters equal the statement, item by item; joints may land off the canvas and stay as they are
    geometry = _geometries(rng, 4)
    for H, W in ((256, 192), (512, 320)):
        got = jitter_keypoints(kp, geometry, H, W)
        for i in range(4):
            assert got[i].tobytes() == JR.keypoints(kp[i], tuple(geometry[i].tolist()), H, W).tobytes(), i
    big = jitter_keypoints(kp, np.tile((1.5, 0.0, 48.0, 64.0), (4, 1)), 256, 192)
    assert (big[..., 0] > 192).any() and (big[..., 1] > 256).any()
    # scale and shift: the centre moves by the shift alone
    centre = np.zeros([1, 18, 3])
    centre[0, :, 0], centre[0, :, 1], centre[0, :, 2] = 95.5, 127.5, 1.0
    moved = jitter_keypoints(centre, [(1.3, 17.0, 5.0, -3.0)], 256, 192)
    assert np.allclose(moved[0, :, 0], 100.5, atol=1e-9) and np.allclose(moved[0, :, 1], 124.5, atol=1e-9)


# ---- the draws ----

FULL = dict(scale=0.5, rotate=45.0, shift=0.25, colour=0.5)


def test_draws_depend_on_seed_and_position_only():
    from training.tryon_batch import jitter_parameters, jitter_uniforms
    g1, c1 = jitter_parameters(FULL, 3, [0, 1, 2, 3, 4, 5], 256, 192)
    assert g1.dtype == np.float64 and g1.shape == (6, 4) and c1.dtype == np.float64 and c1.shape == (6, 3)
    # whatever else is in the batch, whatever the order, one position at a time
    g2, c2 = jitter_parameters(FULL, 3, [5, 2], 256, 192)
    assert g2.tobytes() == g1[[5, 2]].tobytes() and c2.tobytes() == c1[[5, 2]].tobytes()
    g3, c3 = jitter_parameters(FULL, 3, torch.tensor([4]), 256, 192)
    assert g3.tobytes() == g1[[4]].tobytes() and c3.tobytes() == c1[[4]].tobytes()
    # another seed or another position is another draw, and (seed, position) is not (position, seed)
    assert not np.array_equal(jitter_parameters(FULL, 4, [0], 256, 192)[0], g1[[0]])
    assert len({g1[i].tobytes() for i in range(6)}) == 6
    assert not np.array_equal(jitter_uniforms(1, 2), jitter_uniforms(2, 1))
    # the statement's draws, restated
    for t in (0, 1, 7, 2 ** 40):
        geometry, tone = JR.parameters(FULL, 3, t, 256, 192)
        g, c = jitter_parameters(FULL, 3, [t], 256, 192)
        assert tuple(g[0].tolist()) == geometry and tuple(c[0].tolist()) == tone
    u = jitter_uniforms(0, 0)
    assert u.shape == (7,) and u.dtype == np.float64 and u.tolist() == JR.uniforms(0, 0)


def test_changing_one_strength_leaves_the_other_parameters():
    from training.tryon_batch import jitter_parameters
    positions = np.arange(16)
    base_g, base_c = jitter_parameters(FULL, 0, positions, 256, 192)
    columns = dict(scale=[('g', 0)], rotate=[('g', 1)], shift=[('g', 2), ('g', 3)], colour=[('c', 0), ('c', 1), ('c', 2)])
    for name, own in columns.items():
        for value in (0.0, FULL[name] / 2):
            spec = dict(FULL, **{name: value})
            g, c = jitter_parameters(spec, 0, positions, 256, 192)
            for which, got, base in (('g', g, base_g), ('c', c, base_c)):
                for col in range(got.shape[1]):
                    if (which, col) in own:
                        assert not np.array_equal(got[:, col], base[:, col]), (name, which, col)
                    else:
                        assert got[:, col].tobytes() == base[:, col].tobytes(), (name, which, col)
    # a strength of zero is that parameter's identity
    g, c = jitter_parameters(dict(scale=0.2), 0, positions, 256, 192)
    assert not g[:, 1:].any() and np.array_equal(c, np.tile(JR.IDENTITY_TONE, (16, 1))) and (g[:, 0] != 1).all()
    # the shift is a fraction of each side
    g512, _ = jitter_parameters(FULL, 0, positions, 512, 320)
    assert np.allclose(g512[:, 2] * 192, base_g[:, 2] * 320, rtol=1e-15) and np.allclose(g512[:, 3] * 256, base_g[:, 3] * 512, rtol=1e-15)


def test_parameters_stay_inside_their_ranges():
    from training.tryon_batch import jitter_parameters
    H, W = 256, 192
    g, c = jitter_parameters(FULL, 1, np.arange(1000), H, W)
    assert (g[:, 0] >= 1 / 1.5).all() and (g[:, 0] <= 1.5).all() and g[:, 0].min() < 0.7 and g[:, 0].max() > 1.4
    assert (np.abs(g[:, 1]) <= 45).all() and np.abs(g[:, 1]).max() > 40
    assert (np.abs(g[:, 2]) <= 0.25 * W).all() and (np.abs(g[:, 3]) <= 0.25 * H).all() and np.abs(g[:, 3]).max() > 0.2 * H
    assert (c[:, :2] >= 1 / 1.5).all() and (c[:, :2] <= 1.5).all()
    assert (np.abs(c[:, 2]) <= 32).all() and np.abs(c[:, 2]).max() > 28
    # both signs, and centred: the geometric mean of the scale is 1
    assert (g[:, 1] < 0).sum() > 400 and (g[:, 1] > 0).sum() > 400 and abs(np.log(g[:, 0]).mean()) < 0.03


def test_spec_refusals():
    from training.tryon_batch import JITTER_RANGES, jitter_parameters, jitter_spec
    assert JITTER_RANGES == dict(scale=0.5, rotate=45.0, shift=0.25, colour=0.5)
    assert jitter_spec(dict(rotate=5)) == dict(scale=0.0, rotate=5.0, shift=0.0, colour=0.0)
    assert jitter_spec(FULL) == FULL
    for bad, words in ((dict(zoom=0.1), "unknown name 'zoom'"), (dict(scale=0.6), 'scale=0.6 is outside 0..0.5'),
                       (dict(rotate=-1), 'rotate=-1 is outside 0..45'), (dict(shift=float('nan')), 'shift=nan is outside'),
                       (dict(colour=0.0), 'no positive value'), ({}, 'no positive value')):
        with pytest.raises(ValueError, match=words):
            jitter_spec(bad)
    with pytest.raises(ValueError, match='unknown name'):
        jitter_parameters(dict(tilt=1), 0, [0], 256, 192)


# ---- the positions the loop attaches ----

def _fake_loader(batches, n):
    return [dict(raw_idx=torch.arange(n)) for _ in range(batches)]


def test_positions_of_two_ranks_interleave():
    from training.training_loop_wo_flow_fullbody import _numbered_batches
    for skip in (0, 4, 5):
        ranks = [[b['jitter'] for b in _numbered_batches(_fake_loader(3, 2), dict(scale=0.1), 9, 2, rank, skip)] for rank in (0, 1)]
        assert all(j['seed'] == 9 and j['spec'] == dict(scale=0.1) for r in ranks for j in r)
        assert all(j['positions'].dtype == np.int64 and j['positions'].shape == (2,) for r in ranks for j in r)
        merged = sorted(int(t) for r in ranks for j in r for t in j['positions'])
        assert merged == list(range(skip, skip + 12)), (skip, merged)
        for rank, r in enumerate(ranks):
            mine = [int(t) for j in r for t in j['positions']]
            assert mine == sorted(mine) and all(t % 2 == rank for t in mine)
    # one rank: batch after batch
    got = [j['jitter']['positions'].tolist() for j in _numbered_batches(_fake_loader(2, 3), dict(scale=0.1), 0, 1, 0, 0)]
    assert got == [[0, 1, 2], [3, 4, 5]]


class _RawBuilder:
    """Stands in for the GPU builder: the numbered raw batch is what ``_data_batches`` yields."""
    def __init__(self, device):
        pass

    def build(self, raw):
        return raw


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return tryon_tree.make_tree(tmp_path_factory.mktemp('jitter_cpu'))


def _batches(monkeypatch, tree, count, **kwargs):
    from training import training_loop_wo_flow_fullbody as L
    from training import tryon_batch
    monkeypatch.setattr(tryon_batch, 'builder_for', lambda training_set, device: _RawBuilder(device))
    args = dict(num_gpus=1, rank=0, batch_size=2, random_seed=0, device='cpu',
                training_set_kwargs=dict(class_name='training.dataset.UvitonDatasetFull', path=tree), data_loader_kwargs=dict(num_workers=0))
    args.update(kwargs)
    _, _, batches = L._data_batches(**args)
    return [next(batches) for _ in range(count)]


def test_data_batches_number_the_stream_and_a_start_at_k_goes_on_from_k(monkeypatch, tree):
    spec = dict(rotate=10.0)
    whole = _batches(monkeypatch, tree, 5, people_jitter=spec)
    assert [b['jitter']['positions'].tolist() for b in whole] == [[0, 1], [2, 3], [4, 5], [6, 7], [8, 9]]
    assert whole[0]['jitter']['spec'] == dict(scale=0.0, rotate=10.0, shift=0.0, colour=0.0) and whole[0]['jitter']['seed'] == 0
    for k in (4, 3):
        later = _batches(monkeypatch, tree, 2, people_jitter=spec, cur_nimg=k)
        assert [b['jitter']['positions'].tolist() for b in later] == [[k, k + 1], [k + 2, k + 3]]
        stream = torch.cat([b['raw_idx'] for b in whole]).tolist()
        assert torch.cat([b['raw_idx'] for b in later]).tolist() == stream[k:k + 4]
    # two ranks: the people and the positions of the one stream, dealt in turn
    ranks = [_batches(monkeypatch, tree, 2, people_jitter=spec, num_gpus=2, rank=r, batch_size=4, cur_nimg=2) for r in (0, 1)]
    stream = torch.cat([b['raw_idx'] for b in whole]).tolist()
    for r in (0, 1):
        for b in ranks[r]:
            assert [stream[t] for t in b['jitter']['positions'].tolist()] == b['raw_idx'].tolist()
    assert sorted(t for r in ranks for b in r for t in b['jitter']['positions'].tolist()) == list(range(2, 10))
    # without the option a batch is what it was
    plain = _batches(monkeypatch, tree, 2)
    assert all('jitter' not in b for b in plain)
    assert sorted(plain[0]) == ['erase_hw', 'erase_masks', 'image', 'keypoints', 'parsing', 'raw_idx']
    with pytest.raises(ValueError, match='unknown name'):
        _batches(monkeypatch, tree, 1, people_jitter=dict(spin=1))


def test_builders_take_a_batch_without_jitter_as_it_is():
    from training.tryon_batch import jitter_batch
    image, parsing = torch.zeros([2, 4, 3, 3], dtype=torch.uint8), torch.zeros([2, 4, 3], dtype=torch.uint8)
    kp = np.zeros([2, 18, 3])
    got = jitter_batch(dict(xflip=torch.ones(2, dtype=torch.uint8)), image, parsing, kp)
    assert got[0] is image and got[1] is parsing and got[2] is kp


# ---- the command line ----

@pytest.fixture(scope='module')
def cli_tree(tmp_path_factory):
    return make_cli_tree(tmp_path_factory.mktemp('jitter_cli'))


def _options(output):
    text = output[output.index('Training options:') + len('Training options:'):output.index('Output directory:')]
    return json.loads(text)


def _run(tree, outdir, *extra):
    import train_wo_flow_fullbody as T
    return CliRunner().invoke(T.main, ['--outdir', str(outdir), '--data', tree, '--dry-run', *extra])


def test_jitter_people_option(cli_tree, tmp_path):
    import inspect
    from training.training_loop_wo_flow_fullbody import training_loop
    plain = _run(cli_tree, tmp_path / 'runs', '--cfg', 'fashion')
    on = _run(cli_tree, tmp_path / 'runs', '--cfg', 'fashion', '--jitter-people', 'scale=0.1, rotate=5,colour=0.25')
    assert plain.exit_code == 0 and on.exit_code == 0, (plain.output, on.output)
    a, b = _options(plain.output), _options(on.output)
    assert 'people_jitter' not in a and '-jitterpeople' not in plain.output and 'Jittered people:    False' in plain.output
    # a keyword of the loop of its own, not of the data set
    assert b.pop('people_jitter') == dict(scale=0.1, rotate=5.0, shift=0.0, colour=0.25)
    assert 'people_jitter' in inspect.signature(training_loop).parameters
    assert not any('jitter' in k for k in b['training_set_kwargs']) and b['training_set_kwargs'] == a['training_set_kwargs']
    name = os.path.basename(a.pop('run_dir'))
    assert os.path.basename(b.pop('run_dir')) == name.replace('-fashion', '-jitterpeople-fashion') and '-jitterpeople-fashion' in on.output
    assert b == a
    assert 'Jittered people:    scale=0.1,rotate=5,shift=0,colour=0.25' in on.output
    # with --mirror-people: mirror first in the name as in the batch
    both = _run(cli_tree, tmp_path / 'runs', '--cfg', 'fashion', '--mirror-people', 'true', '--jitter-people', 'shift=0.25')
    assert both.exit_code == 0, both.output
    got = _options(both.output)
    assert got['training_set_kwargs']['mirror_people'] is True and got['people_jitter']['shift'] == 0.25
    assert '-mirrorpeople-jitterpeople-fashion' in got['run_dir']


@pytest.mark.parametrize('spec,words', [
    ('zoom=0.1', "unknown name 'zoom'"), ('scale=0.1,tilt=3', "unknown name 'tilt'"), ('scale=0.51', 'scale=0.51 is outside 0..0.5'),
    ('rotate=46', 'rotate=46.0 is outside 0..45'), ('shift=-0.1', 'shift=-0.1 is outside 0..0.25'), ('colour=0.6', 'colour=0.6 is outside 0..0.5'),
    ('scale=0,rotate=0', 'no positive value'), ('scale', "'scale' is not name=value"), ('', "'' is not name=value"),
    ('scale=much', 'scale=much is not a number'), ('scale=0.1,scale=0.2', 'scale is given twice')])
def test_jitter_people_refusals(cli_tree, tmp_path, spec, words):
    res = _run(cli_tree, tmp_path / 'runs', '--cfg', 'fashion', '--jitter-people', spec)
    assert res.exit_code != 0 and '--jitter-people' in res.output and words in res.output, res.output


def test_continue_keeps_the_option_and_refuses_it_again(cli_tree, tmp_path):
    from training import train_state
    res = _run(cli_tree, tmp_path / 'runs', '--cfg', 'fashion', '--batch', '2', '--kimg', '5', '--jitter-people', 'scale=0.2,shift=0.05')
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
    assert got['people_jitter'] == dict(scale=0.2, rotate=0.0, shift=0.05, colour=0.0)
    assert 'Jittered people:    scale=0.2,rotate=0,shift=0.05,colour=0' in res.output
    name = os.path.basename(got['run_dir'])
    assert '-jitterpeople-fashion-' in name and name.endswith('-continue000000')
    res = _run(cli_tree, tmp_path / 'out', '--continue', str(run_dir), '--jitter-people', 'scale=0.2,shift=0.05')
    assert res.exit_code != 0 and '--jitter-people cannot be given with --continue' in res.output, res.output


# ---- scoring never sees jittered people ----

@pytest.mark.parametrize('metric', ['recon_full', 'recon2k'])
def test_scores_build_their_batches_without_the_option(monkeypatch, tree, metric):
    """The option is no data-set keyword, so no score can inherit it from a run's training_set_kwargs; and the batches the
    reconstruction metric hands its builder carry no ``jitter`` (and would be refused as a data-set keyword)."""
    from metrics import metric_main, reconstruction
    from training import tryon_batch
    seen = []

    class Done(Exception):
        pass

    class Builder:
        def build(self, raw):
            seen.append(sorted(raw))
            raise Done
    monkeypatch.setattr(tryon_batch, 'builder_for', lambda dataset, device: Builder())
    monkeypatch.setattr(reconstruction, 'new_partials', lambda *args: None)
    kwargs = dict(class_name='training.dataset.UvitonDatasetFull', path=tree, use_labels=False, max_size=None, xflip=False)
    with pytest.raises(Done):
        metric_main.calc_metric(metric, G=torch.nn.Identity(), dataset_kwargs=kwargs, num_gpus=1, rank=0, device=torch.device('cpu'))
    assert seen == [['erase_hw', 'erase_masks', 'image', 'keypoints', 'parsing', 'raw_idx']]
    with pytest.raises(TypeError):
        metric_main.calc_metric(metric, G=torch.nn.Identity(), dataset_kwargs=dict(kwargs, people_jitter=dict(scale=0.1)), num_gpus=1,
                                rank=0, device=torch.device('cpu'))
