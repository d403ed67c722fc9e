"""The swapped try-on metric on the host: the registry, the block partition of metrics/tryon_swapped.py, the training
command's --metrics, and ``swap_outfits.attach`` with explicit source tables.  No GPU and no library load."""
import itertools
import json
import os

import numpy as np
import pytest
import torch
from click.testing import CliRunner

from train_grid_tree import make_tree

COMMAND = ('--cfg', 'fashion', '--batch', '4', '--kimg', '5', '--l1_weight', '40', '--mask_weight', '20')


# ---- a. the registry ----

def test_the_metrics_are_registered_after_the_recon_ones():
    from metrics import metric_main
    assert metric_main.is_valid_metric('tryon_full') and metric_main.is_valid_metric('tryon2k')
    assert metric_main.list_valid_metrics()[:2] == ['recon_full', 'recon2k']
    assert not metric_main.is_valid_metric('tryon') and not metric_main.is_valid_metric('tryon_fidelity')
    # two families: list_valid_metrics keeps listing the paired metrics, list_metrics names everything a command takes
    assert metric_main.list_unpaired_metrics() == ['tryon_full', 'tryon2k']
    assert metric_main.list_metrics() == ['recon_full', 'recon2k', 'tryon_full', 'tryon2k']
    with pytest.raises(ValueError, match='valid metrics: recon_full, recon2k, tryon_full, tryon2k'):
        metric_main.calc_metric('tryon', G=None, dataset_kwargs={}, num_gpus=1, rank=0, device=torch.device('cpu'))


def test_the_scoring_command_names_every_metric():
    import calc_metrics
    res = CliRunner().invoke(calc_metrics.calc_metrics, ['--network', 'none.pkl', '--metrics', 'tryon2k,nope'])
    assert res.exit_code != 0 and 'unknown metric nope' in res.output and 'valid metrics: recon_full, recon2k, tryon_full, tryon2k' in res.output
    assert 'tryon_full, tryon2k' in CliRunner().invoke(calc_metrics.calc_metrics, ['--help']).output


def test_the_metrics_force_their_data_set_options(monkeypatch):
    """What the two names hand on: the people as photographed, no erase mask (and no strokes specification, which the data set
    refuses without ``erase_masks='strokes'``), the whole tree or the 2000 items of seed 0."""
    from metrics import metric_main, tryon_swapped
    seen = []
    monkeypatch.setattr(tryon_swapped, 'compute', lambda opts, prefix: (seen.append((prefix, dict(opts.dataset_kwargs))), {prefix + '_x': 1.0})[1])
    recorded = dict(class_name='training.dataset.UvitonDatasetFull', path='t', xflip=True, mirror_people=True, erase_masks='strokes',
                    erase_strokes=dict(count=3), max_size=7, random_seed=5)
    for name in ('tryon_full', 'tryon2k'):
        r = metric_main.calc_metric(name, G=None, dataset_kwargs=recorded, num_gpus=1, rank=0, device=torch.device('cpu'))
        assert r.metric == name and dict(r.results) == {name + '_x': 1.0}
    common = dict(class_name='training.dataset.UvitonDatasetFull', path='t', xflip=False, mirror_people=False, erase_masks='none')
    assert seen[0] == ('tryon_full', dict(common, max_size=None, random_seed=5))
    assert seen[1] == ('tryon2k', dict(common, max_size=2000, random_seed=0))
    assert recorded['erase_masks'] == 'strokes' and recorded['max_size'] == 7          # the caller's options are not written to


# ---- b. the block partition ----

@pytest.mark.parametrize('M,B,G', list(itertools.product((2, 3, 5, 9, 17), (1, 2, 4, 9, 32), (1, 2, 8))))
def test_blocks(M, B, G):
    from metrics.tryon_swapped import blocks
    scored = []
    for rank in range(G):
        mine = blocks(M, B, G, rank)
        for rows, load, upper_src, lower_src in mine:
            assert rows == list(range(rows[0], rows[0] + len(rows))) and rows[0] % B == 0 and (rows[0] // B) % G == rank
            assert 1 <= len(rows) <= B and (len(rows) == B or rows[-1] == M - 1)
            assert load[:len(rows)] == rows and len(set(load)) == len(load) <= min(B + 1, M) and all(0 <= i < M for i in load)
            assert len(upper_src) == len(lower_src) == len(load) and upper_src == lower_src
            for j, i in enumerate(rows):
                assert load[upper_src[j]] == (i + 1) % M and load[lower_src[j]] == (i + 1) % M
            for j in range(len(rows), len(load)):                   # the extra person: its own garments, and it is the last row's donor
                assert upper_src[j] == j and load[j] == (rows[-1] + 1) % M
            scored += rows
        if M <= B:
            assert len(mine) == (1 if rank == 0 else 0)
            if mine:
                assert mine[0][0] == mine[0][1] == list(range(M))
    assert sorted(scored) == list(range(M))                         # every item exactly once over the ranks


def test_blocks_refuse_a_single_item():
    from metrics.tryon_swapped import blocks
    for M in (0, 1):
        with pytest.raises(ValueError, match='at least 2 items.*: %d' % M):
            blocks(M, 4, 1, 0)


def test_a_tree_of_one_person_is_refused_by_name(monkeypatch):
    import dnnlib
    from metrics import metric_utils, tryon_swapped
    monkeypatch.setattr(dnnlib.util, 'construct_class_by_name', lambda **kwargs: [None])
    opts = metric_utils.MetricOptions(G=None, dataset_kwargs=dict(class_name='x', path='/data/one_person'), device=torch.device('cpu'))
    with pytest.raises(ValueError, match='/data/one_person has 1'):
        tryon_swapped.compute_partials(opts)


def test_an_item_nobody_scored_is_an_error():
    from metrics import tryon_fidelity, tryon_swapped
    p = tryon_fidelity.new_partials(3)
    p[:, 0, 3] = 30                                                  # keep bytes: scored; the garment regions stay empty
    p[:, 0, 0] = 60
    r = tryon_swapped.finish(p, 'tryon_full', 100)
    assert len(r) == 18 and r['tryon_full_keep_pairs'] == 3 and r['tryon_full_upper_pairs'] == 0 and r['tryon_full_upper_share'] == 0
    assert np.isnan(r['tryon_full_upper_l1']) and np.isnan(r['tryon_full_lower_ssim']) and np.isnan(r['tryon_full_keep_ssim'])
    assert r['tryon_full_keep_l1'] == pytest.approx(2 / 255.0, rel=1e-12) and r['tryon_full_keep_share'] == pytest.approx(0.1, rel=1e-12)
    p[1] = 0
    with pytest.raises(ValueError, match='1 of 3 items were not scored'):
        tryon_swapped.finish(p, 'tryon_full', 100)


# ---- c. the training command ----

@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return make_tree(tmp_path_factory.mktemp('tryon_metric_cli'))


def _options(output):
    text = output[output.index('Training options:') + len('Training options:'):output.index('Output directory:')]
    return json.loads(text)


def _run(tree, outdir, *extra):
    import train_wo_flow_fullbody as T
    return CliRunner().invoke(T.main, ['--outdir', str(outdir), '--data', tree, '--dry-run', *extra])


def test_the_command_takes_the_metric(tree, tmp_path):
    res = _run(tree, tmp_path / 'runs', *COMMAND, '--metrics', 'tryon2k')
    assert res.exit_code == 0, res.output
    assert _options(res.output)['metrics'] == ['tryon2k']
    res = _run(tree, tmp_path / 'runs', *COMMAND, '--metrics', 'recon2k,tryon2k,tryon_full', '--metrics_data', tree)
    assert res.exit_code == 0, res.output
    o = _options(res.output)
    assert o['metrics'] == ['recon2k', 'tryon2k', 'tryon_full'] and o['metric_set_kwargs']['path'] == tree
    res = _run(tree, tmp_path / 'runs', *COMMAND, '--metrics', 'fid50k_full')
    assert res.exit_code != 0 and 'metric call commented out' in res.output and 'refused: fid50k_full' in res.output, res.output
    # nothing changes for a run without the names
    plain, recon = _run(tree, tmp_path / 'runs', *COMMAND), _run(tree, tmp_path / 'runs', *COMMAND, '--metrics', 'recon_full')
    assert plain.exit_code == 0 and recon.exit_code == 0
    assert _options(plain.output)['metrics'] == [] and _options(recon.output)['metrics'] == ['recon_full']
    assert 'tryon_full' not in plain.output + recon.output and 'tryon2k' not in plain.output + recon.output


def test_continue_takes_the_metric(tree, tmp_path):
    from training import train_state
    res = _run(tree, tmp_path / 'runs', *COMMAND)
    assert res.exit_code == 0, res.output
    options = _options(res.output)
    assert options['metrics'] == []
    run_dir = tmp_path / 'runs' / os.path.basename(options['run_dir'])
    os.makedirs(run_dir)
    empty = dict(cur_nimg=0, batch_idx=0, cur_tick=1, elapsed_sec=0.0, num_gpus=1, batch_size=4, batch_gpu=4, random_seed=0,
                 options=json.dumps(options, indent=2), G={}, D={}, G_ema={}, opt={}, grid_z=torch.zeros([0, 0]), ranks=[])
    train_state.save_state(str(run_dir / 'training-state-000000.pt'), None, empty)
    res = _run(tree, tmp_path / 'out', '--continue', str(run_dir), '--metrics', 'tryon2k')
    assert res.exit_code == 0, res.output
    assert _options(res.output)['metrics'] == ['tryon2k']
    res = _run(tree, tmp_path / 'out', '--continue', str(run_dir), '--metrics', 'fid50k_full')
    assert res.exit_code != 0 and '--metrics: not evaluated: fid50k_full' in res.output, res.output


# ---- d. attach ----

class _Builder:
    lower_parts = (6, 7, 8, 9)


def _attach(monkeypatch, n, swap, keep_stages=False):
    """``swap_outfits.attach`` on stand-in stages with ``swap_tensors`` mocked: (the call it made, the tensors, the stages)."""
    from training import swap_outfits
    calls = []
    def mocked(stages, back, valid, lower_parts, upper_src, lower_src, composites=None):
        calls.append(dict(stages=stages, back=back, valid=valid, lower_parts=lower_parts, upper_src=np.asarray(upper_src).tolist(),
                          lower_src=np.asarray(lower_src).tolist(), composites=composites))
        if composites is not None:
            composites.update(swap_denorm_upper='U', swap_denorm_lower='L')
        return {k: k for k in swap_outfits.SWAP_OUTPUTS}
    monkeypatch.setattr(swap_outfits, 'swap_tensors', mocked)
    stages = dict(retain_mask=torch.zeros([n, 4, 4], dtype=torch.uint8))
    tensors = swap_outfits.attach(dict(real_img='r'), stages, 'back', 'valid', _Builder(), swap, **(dict(keep_stages=True) if keep_stages else {}))
    return calls, tensors, stages


@pytest.mark.parametrize('n,group,region', [(4, 2, 'fullbody'), (4, 4, 'upperbody'), (6, 3, 'lowerbody'), (2, 2, 'fullbody')])
def test_explicit_tables_are_the_donor_rule_when_they_name_it(monkeypatch, n, group, region):
    from training import swap_outfits
    upper_src, lower_src = swap_outfits.source_tables(n, group, region)
    by_rule, t_rule, s_rule = _attach(monkeypatch, n, dict(region=region, group=group))
    by_table, t_table, s_table = _attach(monkeypatch, n, dict(upper_src=upper_src, lower_src=lower_src))
    assert len(by_rule) == len(by_table) == 1
    a, b = by_rule[0], by_table[0]
    assert a['upper_src'] == b['upper_src'] == upper_src.tolist() and a['lower_src'] == b['lower_src'] == lower_src.tolist()
    assert all(a[k] == b[k] for k in ('back', 'valid', 'lower_parts')) and a['composites'] is None and b['composites'] is None
    assert list(t_rule) == list(t_table) == ['real_img'] + swap_outfits.SWAP_KEYS
    assert t_table['swap_keep'] is s_table['retain_mask'] and list(s_rule) == list(s_table) == ['retain_mask']
    # lists serve as arrays do, and kept stages receive the two composites
    calls, _, stages = _attach(monkeypatch, n, dict(upper_src=upper_src.tolist(), lower_src=lower_src.tolist()), keep_stages=True)
    assert calls[0]['upper_src'] == upper_src.tolist() and calls[0]['composites'] is stages
    assert list(stages) == ['retain_mask'] + list(swap_outfits.SWAP_STAGES)


@pytest.mark.parametrize('swap,message', [
    (dict(upper_src=[1, 2, 3], lower_src=[1, 2, 0]), 'upper_src'),
    (dict(upper_src=[1, 2, 0], lower_src=[-1, 2, 0]), 'lower_src'),
    (dict(upper_src=[1, 2], lower_src=[1, 2, 0]), 'upper_src'),
    (dict(upper_src=[1, 2, 0], lower_src=[1, 2, 0, 0]), 'lower_src'),
    (dict(upper_src=[1, 2, 0]), 'upper_src= and lower_src='),
    (dict(upper_src=[1, 2, 0], lower_src=[1, 2, 0], group=3), 'upper_src= and lower_src='),
])
def test_tables_outside_the_batch_are_refused_before_any_launch(monkeypatch, swap, message):
    from training import swap_outfits
    monkeypatch.setattr(swap_outfits, 'swap_tensors', lambda *a, **k: pytest.fail('launched'))
    tensors = dict(real_img='r')
    with pytest.raises(ValueError, match=message):
        swap_outfits.attach(tensors, dict(retain_mask=torch.zeros([3, 4, 4], dtype=torch.uint8)), 'back', 'valid', _Builder(), swap)
    assert list(tensors) == ['real_img']
    with pytest.raises(ValueError, match='groups of at least 2'):             # the donor rule's own refusals stay
        swap_outfits.attach(tensors, dict(retain_mask=torch.zeros([3, 4, 4], dtype=torch.uint8)), 'back', 'valid', _Builder(), dict(group=1))
