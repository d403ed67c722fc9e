"""People fitted to the canvas without a GPU (--fit-people; include/pasta_hip.h, pasta_fit_people_u8): the numpy
statement (tests/fit_ref.py) against PIL byte for byte, the fitted rectangle and its limits, the label rule with its ties, the
joints, the host's tap tables against the statement's, the data sets and collate functions on ragged trees, and the command
line's option."""
import json
import os

import numpy as np
import PIL.Image
import pytest
import torch
from click.testing import CliRunner

import fit_ref as R
import fit_tree as T
from train_grid_tree import make_tree as make_cli_tree
from tryon_512_train_tree import make_512_train_tree
from tryon_pairs_tree import make_pair_tree
from tryon_tree import make_tree

# source h x w -> fitted Hc x Wc: the thirteen shape pairs the rule was checked on
SHAPES = [((1024, 768), (256, 192)), ((1101, 743), (256, 173)), ((512, 320), (256, 160)), ((300, 200), (256, 171)), ((77, 53), (256, 176)),
          ((641, 480), (512, 320)), ((2048, 1536), (512, 320)), ((256, 192), (256, 192)), ((256, 100), (256, 100)), ((333, 192), (256, 148)),
          ((100, 75), (512, 320)), ((19, 13), (23, 16)), ((16, 40), (7, 17))]
PIL_FILTERS = {'box': PIL.Image.BOX, 'bilinear': PIL.Image.BILINEAR}


@pytest.mark.parametrize('src,dst', SHAPES)
def test_the_statement_equals_pil(src, dst):
    rng = np.random.default_rng(src[0] * 4096 + src[1])
    for channels in (3, 1):
        a = rng.integers(0, 256, [*src, 3] if channels == 3 else list(src), dtype=np.uint8)
        for name, pil in PIL_FILTERS.items():
            want = np.array(PIL.Image.fromarray(a).resize((dst[1], dst[0]), pil))
            got = R.resample(a, dst[0], dst[1], name)
            assert got.shape == want.shape and np.array_equal(got, want), (src, dst, name, channels, int((got != want).sum()))


@pytest.mark.parametrize('src,dst', SHAPES)
def test_the_hosts_tap_tables_are_the_statements(src, dst):
    from training.tryon_batch import fit_taps
    for n_in, n_out in zip(src, dst):
        for filter in ('box', 'bilinear'):
            xmin, cnt, k = fit_taps(n_in, n_out, filter)
            assert k.shape[1] <= 17 and (filter != 'box' or k.shape[1] <= 9)
            for p, (first, taps) in enumerate(R.taps(n_in, n_out, filter)):
                assert xmin[p] == first and cnt[p] == len(taps) and np.array_equal(k[p, :cnt[p]], taps) and not k[p, cnt[p]:].any()
    assert fit_taps(src[0], dst[0], 'box') is fit_taps(src[0], dst[0], 'box')          # cached per (n_in, n_out, filter)


@pytest.mark.parametrize('h,w,pad,crop', [(1024, 768, (256, 192, 0, 0), (256, 192, 0, 0)), (512, 320, (256, 160, 0, 16), (307, 192, -25, 0)),
                                          (1101, 743, (256, 173, 0, 9), None), (200, 190, None, None), (256, 192, (256, 192, 0, 0), (256, 192, 0, 0))])
def test_fitted_rectangle(h, w, pad, crop):
    from training.tryon_batch import fit_rectangle
    for mode, stated in (('pad', pad), ('crop', crop)):
        want = R.rectangle(h, w, 256, 192, mode)
        assert fit_rectangle(h, w, 256, 192, mode) == want and (stated is None or want == stated)
        Hc, Wc, oy, ox = want
        if mode == 'pad':
            assert Hc <= 256 and Wc <= 192 and (Hc == 256 or Wc == 192) and 0 <= oy <= 256 - Hc and 0 <= ox <= 192 - Wc
        else:
            assert Hc >= 256 and Wc >= 192 and (Hc == 256 or Wc == 192) and oy <= 0 and ox <= 0 and oy + Hc >= 256 and ox + Wc >= 192


def test_label_rule():
    rng = np.random.default_rng(0)
    lab = rng.integers(0, 20, [31, 17], dtype=np.uint8)
    out, tied = R.label_mode(lab, 31, 17)
    assert np.array_equal(out, lab) and tied == 0                                       # the identity is a copy
    for f in (2, 3, 8):
        blocks = rng.integers(0, 256, [9, 7], dtype=np.uint8)
        out, tied = R.label_mode(blocks.repeat(f, 0).repeat(f, 1), 9, 7)
        assert np.array_equal(out, blocks) and tied == 0
    total = 0
    for (h, w), (Hc, Wc), seed in (((77, 53), (64, 44), 1), ((81, 24), (40, 24), 2), ((10, 6), (40, 24), 3)):
        src = R.voronoi_labels(h, w, seed)
        out, tied = R.label_mode(src, Hc, Wc)
        assert set(np.unique(out)) <= set(np.unique(src))
        total += tied
    assert total > 0                                                                    # the tie rule is exercised
    # a constructed tie of two labels: 2 -> 1 along both axes, each label on two of the four pixels.  The centre pixel of output
    # (r, c) is source ((2 r + 1) 4 // 4, ...) = (2 r + 1, 2 c + 1): its label wins, the smaller label or not
    src = np.array([[3, 9, 9, 3], [9, 3, 3, 9], [5, 5, 1, 1], [7, 7, 2, 2]], np.uint8)
    out, tied = R.label_mode(src, 2, 2)
    assert tied == 4 and out.tolist() == [[3, 9], [7, 2]]
    # a tie the centre pixel's label is no part of: the smallest tied label.  3 -> 1: the centre is source (1, 1)
    src = np.array([[4, 4, 4], [8, 6, 8], [8, 2, 2]], np.uint8)
    out, tied = R.label_mode(src, 1, 1)
    assert tied == 1 and out.tolist() == [[4]]


def test_joints():
    from training.tryon_batch import fit_keypoints
    rng = np.random.default_rng(0)
    kp = np.concatenate([rng.uniform(-20, 300, [3, 18, 2]), rng.uniform(0.1, 1.0, [3, 18, 1])], axis=2)
    kp[1, 4] = (123.456, 78.9, 0.0999)
    kp[2, 5] = (np.nan, np.inf, 0.0)
    same = fit_keypoints(kp, [(256, 192)] * 3, [(256, 192, 0, 0)] * 3)
    assert same.tobytes() == kp.tobytes()                                                # the identity keeps values
    hw, rects = [(512, 320), (300, 250), (100, 75)], [(256, 160, 0, 16), (307, 256, -25, -32), (256, 192, 0, 0)]
    got = fit_keypoints(kp, hw, rects)
    for i in range(3):
        assert np.array_equal(got[i], R.keypoints(kp[i], *hw[i], rects[i]), equal_nan=True)
    assert got[1, 4].tobytes() == kp[1, 4].tobytes() and got[2, 5].tobytes() == kp[2, 5].tobytes()       # below 0.1: the bits
    # one joint by hand: 512 x 320 padded into 256 x 160 at column 16: x' = 100 * 0.5 + ((0.25 - 0.5) + 16), y' = 200 * 0.5 - 0.25
    one = fit_keypoints(np.tile(np.array([100.0, 200.0, 0.5]), (1, 18, 1)), [(512, 320)], [(256, 160, 0, 16)])
    assert one[0, 0].tolist() == [65.75, 99.75, 0.5]


@pytest.fixture(scope='module')
def trees(tmp_path_factory):
    root = tmp_path_factory.mktemp('fit_cpu')
    plain = {256: make_tree(root / 'plain256'), 512: make_512_train_tree(root / 'plain512')}
    sizes = {res: T.ragged_copy(plain[res], root / ('ragged%d' % res)) for res in plain}
    return plain, {res: str(root / ('ragged%d' % res)) for res in plain}, sizes


def _classes():
    from training import dataset as D
    return {256: D.UvitonDatasetFull, 512: D.UvitonDatasetFull_512}


@pytest.mark.parametrize('res,canvas', [(256, (256, 192)), (512, (512, 320))])
def test_a_ragged_tree_opens_with_fit_and_collate_packs_it(trees, res, canvas):
    from training import dataset as D
    _, ragged, sizes = trees
    cls = _classes()[res]
    assert cls.canvas == canvas
    with pytest.raises((ValueError, IOError)):
        D.collate([cls(ragged[res])[i] for i in range(len(sizes[res]))])           # without the option the tree is what it always was
    ds = cls(ragged[res], fit='pad', fit_filter='box', resolution=canvas[0])
    assert ds.resolution == canvas[0] and ds.content_width == canvas[1] and ds.image_shape == [3, canvas[0], canvas[0]] and len(ds) == 5
    with pytest.raises(IOError):
        cls(ragged[res], fit='pad', resolution=canvas[0] + 1)
    samples = [ds[i] for i in range(len(ds))]
    assert sorted(s['image'].shape[:2] for s in samples) == sorted(sizes[res]) and len(set(sizes[res])) == 5
    assert all(s['fit'] == dict(mode='pad', filter='box', canvas=canvas) and s['parsing'].shape == s['image'].shape[:2] for s in samples)
    b = D.collate(samples)
    assert b['fit'] == samples[0]['fit'] and b['image'].dtype == torch.uint8 and b['image'].ndim == 1 and b['parsing'].ndim == 1
    assert b['image_hw'].dtype == torch.int32 and b['image_offsets'].dtype == torch.int64 and b['keypoints'].shape == (5, 18, 3)
    assert b['image'].numel() == 3 * b['parsing'].numel() == 3 * sum(h * w for h, w in sizes[res])
    for s, (h, w), off in zip(samples, b['image_hw'].tolist(), b['image_offsets'].tolist()):
        assert (h, w) == s['parsing'].shape
        assert np.array_equal(b['image'][3 * off:3 * (off + h * w)].numpy().reshape(h, w, 3), s['image'])
        assert np.array_equal(b['parsing'][off:off + h * w].numpy().reshape(h, w), s['parsing'])


def test_a_canvas_size_tree_collated_with_fit_holds_the_same_bytes(trees):
    from training import dataset as D
    plain, _, _ = trees
    for res, cls in _classes().items():
        a = D.collate([cls(plain[res])[i] for i in range(3)])
        b = D.collate([cls(plain[res], fit='crop')[i] for i in range(3)])
        assert b['image'].numpy().tobytes() == a['image'].numpy().tobytes() and b['parsing'].numpy().tobytes() == a['parsing'].numpy().tobytes()
        assert b['image_hw'].tolist() == [list(a['image'].shape[1:3])] * 3 and torch.equal(a['keypoints'], b['keypoints'])
        assert sorted(set(b) - set(a)) == ['fit', 'image_hw', 'image_offsets']


def test_outfits_of_a_ragged_pair_tree_are_packed(tmp_path):
    from training import dataset as D
    plain = make_pair_tree(tmp_path / 'pairs')
    sizes = T.ragged_copy(plain, tmp_path / 'ragged')
    assert len(set(sizes)) > 1
    with pytest.raises(IOError):
        [s for s in D.UvitonDatasetV19_test(str(tmp_path / 'ragged'))]              # a pair of two sizes, as ever
    ds = D.UvitonDatasetV19_test(str(tmp_path / 'ragged'), fit='pad')
    assert ds.resolution == 256 and D.UvitonDatasetV19_test.canvas == D.UvitonOutfits_256_test.canvas == (256, 192)
    assert D.UvitonDatasetFull_512_test.canvas == D.UvitonOutfits_512_test.canvas == (512, 320)
    samples = [ds[i] for i in range(len(ds))]
    assert any(s['image'].shape != s['clothes_image'].shape for s in samples)       # a pair need not match any more
    b = D.collate_region_outfits('fullbody', samples)
    m = len(b['people_name'])
    assert b['fit'] == dict(mode='pad', filter='bilinear', canvas=(256, 192)) and b['people_image'].ndim == 1
    assert b['people_image_hw'].shape == (m, 2) and b['people_image_offsets'].shape == (m,) and b['people_keypoints'].shape == (m, 18, 3)
    by_name = {}
    for s in samples:
        by_name[s['person_name']], by_name[s['clothes_name']] = s['image'], s['clothes_image']
    for name, (h, w), off in zip(b['people_name'], b['people_image_hw'].tolist(), b['people_image_offsets'].tolist()):
        assert np.array_equal(b['people_image'][3 * off:3 * (off + h * w)].numpy().reshape(h, w, 3), by_name[name])


def test_unknown_values_and_the_limits(trees, tmp_path):
    from training import dataset as D
    from training.tryon_batch import fit_limits
    plain, _, _ = trees
    for kwargs in (dict(fit='stretch'), dict(fit='pad', fit_filter='lanczos'), dict(fit_filter='nearest')):
        for cls, args in ((D.UvitonDatasetFull, ()), (D.UvitonDatasetV19_test, ())):
            with pytest.raises(ValueError):
                cls(plain[256], *args, **kwargs)
    # each of the four limits, on canvas (256, 192): taller than 8 Hc, wider than 8 Wc, Hc above 4 h, Wc above 4 w
    cases = {'pad': [(2049, 1536), (63, 47)], 'crop': [(2048, 1537), (63, 48), (64, 47)]}
    assert fit_limits(2048, 1536, 256, 192) is None and fit_limits(64, 48, 256, 192) is None
    assert fit_limits(2049, 10, 256, 192) and fit_limits(10, 1537, 256, 192) and fit_limits(63, 192, 256, 192) and fit_limits(256, 47, 256, 192)
    tree = T.ragged_copy(plain[256], tmp_path / 'limits', factors=((1.0, 1.0),)) and str(tmp_path / 'limits')
    first = T.people(tree)
    zalando = [p for p in first if 'Zalando_256_192' in p[0]][0]
    for mode, shapes in cases.items():
        for h, w in shapes:
            PIL.Image.fromarray(np.zeros([h, w, 3], np.uint8)).save(zalando[0], format='PNG')
            PIL.Image.fromarray(np.zeros([h, w], np.uint8), mode='L').save(zalando[1], format='PNG')
            ds = D.UvitonDatasetFull(tree, fit=mode)
            with pytest.raises(IOError, match=os.path.basename(zalando[0])):
                ds[0]


@pytest.fixture(scope='module')
def cli_tree(tmp_path_factory):
    return make_cli_tree(tmp_path_factory.mktemp('people_cli'))


def _options(output):
    text = output[output.index('Training options:') + len('Training options:'):output.index('Output directory:')]
    return json.loads(text)


def _run(tree, outdir, *extra):
    import train_wo_flow_fullbody as M
    return CliRunner().invoke(M.main, ['--outdir', str(outdir), '--data', tree, '--dry-run', *extra])


def test_the_option_is_recorded_only_when_given_and_continue_keeps_it(cli_tree, tmp_path):
    from training import train_state
    plain = _run(cli_tree, tmp_path / 'runs', '--cfg', 'fashion', '--batch', '2', '--kimg', '5')
    assert plain.exit_code == 0, plain.output
    a = _options(plain.output)
    name = os.path.basename(a.pop('run_dir'))
    assert not any('fit' in k for k in list(a) + list(a['training_set_kwargs'])) and '-fit' not in name and 'Fitted people' not in plain.output
    for extra, filter in ((('--fit-people', 'pad'), 'bilinear'), (('--fit-people', 'crop', '--fit-filter', 'box'), 'box')):
        on = _run(cli_tree, tmp_path / 'runs', '--cfg', 'fashion', '--batch', '2', '--kimg', '5', *extra, '--metrics', 'recon_full', '--metrics_data', cli_tree)
        assert on.exit_code == 0, on.output
        b = _options(on.output)
        assert b['training_set_kwargs'].pop('fit') == extra[1] and b['training_set_kwargs'].pop('fit_filter') == filter
        assert b['metric_set_kwargs']['fit'] == extra[1] and b['metric_set_kwargs']['fit_filter'] == filter
        assert os.path.basename(b.pop('run_dir')) == name.replace('-fashion', '-fit%s-fashion' % extra[1])
        assert 'Fitted people:      %s (%s)\n' % (extra[1], filter) in on.output
        b.pop('metric_set_kwargs'), b.pop('metrics')
        assert b == {k: v for k, v in a.items() if k not in ('metric_set_kwargs', 'metrics')}
    res = _run(cli_tree, tmp_path / 'runs', '--fit-filter', 'box')
    assert res.exit_code != 0 and '--fit-filter needs --fit-people' in res.output
    res = _run(cli_tree, tmp_path / 'runs', '--fit-people', 'stretch')
    assert res.exit_code != 0
    # --continue keeps the recorded option and refuses it again
    on = _run(cli_tree, tmp_path / 'runs', '--cfg', 'fashion', '--batch', '2', '--kimg', '5', '--fit-people', 'pad')
    options = _options(on.output)
    run_dir = tmp_path / 'runs' / os.path.basename(options['run_dir'])
    os.makedirs(run_dir)
    empty = dict(cur_nimg=0, batch_idx=0, cur_tick=1, elapsed_sec=0.0, num_gpus=1, batch_size=2, batch_gpu=2, random_seed=0,
                 options=json.dumps(options, indent=2), G={}, D={}, G_ema={}, opt={}, grid_z=torch.zeros([0, 0]), ranks=[])
    train_state.save_state(str(run_dir / 'training-state-000000.pt'), None, empty)
    res = _run(cli_tree, tmp_path / 'out', '--continue', str(run_dir))
    assert res.exit_code == 0, res.output
    got = _options(res.output)
    assert got['training_set_kwargs']['fit'] == 'pad' and got['training_set_kwargs']['fit_filter'] == 'bilinear'
    assert 'Fitted people:      pad (bilinear)' in res.output
    res = _run(cli_tree, tmp_path / 'out', '--continue', str(run_dir), '--fit-people', 'pad')
    assert res.exit_code != 0 and '--fit-people cannot be given with --continue' in res.output, res.output


def test_calc_metrics_defaults_to_what_the_snapshot_recorded(monkeypatch, cli_tree, tmp_path):
    import calc_metrics
    import legacy
    res = CliRunner().invoke(calc_metrics.calc_metrics, ['--help'])
    assert res.exit_code == 0 and '--fit-people' in res.output and '--fit-filter' in res.output
    pkl = tmp_path / 'network-snapshot-000000.pkl'
    pkl.write_bytes(b'stands in for a snapshot')
    seen = []
    monkeypatch.setattr(calc_metrics, 'subprocess_fn', lambda rank, args, temp_dir: seen.append(dict(args.dataset_kwargs)))

    def run(recorded, *extra):
        monkeypatch.setattr(legacy, 'load_network_pkl', lambda f: dict(training_set_kwargs=dict(
            class_name='training.dataset.UvitonDatasetFull', path=cli_tree, use_labels=False, max_size=9, xflip=False, **recorded)))
        del seen[:]
        res = CliRunner().invoke(calc_metrics.calc_metrics, ['--network', str(pkl), '--verbose', 'false', *extra])
        assert res.exit_code == 0, res.output
        return {k: v for k, v in seen[0].items() if k.startswith('fit')}
    recorded = dict(fit='pad', fit_filter='box')
    assert run({}) == {} and run({}, '--data', cli_tree) == {}
    assert run(recorded) == recorded and run(recorded, '--data', cli_tree) == recorded
    assert run({}, '--fit-people', 'crop') == dict(fit='crop', fit_filter='bilinear')
    assert run(recorded, '--fit-people', 'crop') == dict(fit='crop', fit_filter='box')
    assert run(recorded, '--fit-filter', 'bilinear') == dict(fit='pad', fit_filter='bilinear')


def test_the_try_on_commands_take_the_options():
    import test as test_256
    import test_512
    for command in (test_256.generate_images, test_512.generate_images):
        res = CliRunner().invoke(command, ['--help'])
        assert res.exit_code == 0 and '--fit-people' in res.output and '--fit-filter' in res.output
