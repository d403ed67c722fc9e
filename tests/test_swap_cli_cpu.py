"""``--swap_weight`` and ``--swap-region`` of train_wo_flow_fullbody.py through ``--dry-run``: what they record, that
their absence records nothing, and what they refuse."""
import json
import os

import pytest
import torch
from click.testing import CliRunner

from train_grid_tree import make_tree
from tryon_512_train_tree import make_512_train_tree

COMMAND = ('--cfg', 'fashion', '--batch', '4', '--kimg', '5', '--l1_weight', '40', '--mask_weight', '20')


@pytest.fixture(scope='module')
def trees(tmp_path_factory):
    return {256: make_tree(tmp_path_factory.mktemp('swap_cli_256')), 512: make_512_train_tree(tmp_path_factory.mktemp('swap_cli_512'))}


def _options(output):
    text = output[output.index('Training options:') + len('Training options:'):output.index('Output directory:')]
    return json.loads(text)


def _run(tree, outdir, *extra):
    import train_wo_flow_fullbody as T
    return CliRunner().invoke(T.main, ['--outdir', str(outdir), '--data', tree, '--dry-run', *extra])


@pytest.mark.parametrize('res', [256, 512])
def test_the_options_record_weight_region_and_group(trees, tmp_path, res):
    plain = _run(trees[res], tmp_path / 'runs', *COMMAND)
    swap = _run(trees[res], tmp_path / 'runs', *COMMAND, '--swap_weight', '1', '--swap-region', 'upperbody')
    assert plain.exit_code == 0 and swap.exit_code == 0, (plain.output, swap.output)
    a, b = _options(plain.output), _options(swap.output)
    assert b['cfg']['loss_kwargs']['swap_weight'] == 1 and b['swap_outfits'] == dict(region='upperbody', group=4)
    assert b['run_dir'].endswith('-swap1upperbody') and 'Swapped outfits:    weight 1, upperbody, groups of 4' in swap.output
    # nothing else moved
    b['cfg']['loss_kwargs'].pop('swap_weight')
    b.pop('swap_outfits')
    b['run_dir'] = b['run_dir'][:-len('-swap1upperbody')]
    assert a == b
    # the default region is not named; the group is the per-GPU round
    full = _run(trees[res], tmp_path / 'runs', *COMMAND, '--swap_weight', '0.5', '--gpus', '2')
    assert full.exit_code == 0, full.output
    got = _options(full.output)
    assert got['swap_outfits'] == dict(region='fullbody', group=2) and got['run_dir'].endswith('-swap0.5')


def test_without_the_options_the_command_prints_what_it_printed(trees, tmp_path):
    """Against a run of the same command: absent, and a weight of 0, add no key and no line."""
    plain = _run(trees[256], tmp_path / 'runs', *COMMAND)
    zero = _run(trees[256], tmp_path / 'runs', *COMMAND, '--swap_weight', '0')
    assert plain.exit_code == 0 and zero.exit_code == 0
    assert zero.output == plain.output
    assert 'Swapped outfits' not in plain.output and 'swap_' not in plain.output.replace('swap_cli_', '')
    options = _options(plain.output)
    assert 'swap_outfits' not in options and 'swap_weight' not in options['cfg']['loss_kwargs']


def test_the_refusals(trees, tmp_path):
    res = _run(trees[256], tmp_path / 'runs', *COMMAND, '--swap_weight', '-1')
    assert res.exit_code != 0 and '--swap_weight must be non-negative' in res.output, res.output
    for extra in ((), ('--swap_weight', '0')):
        res = _run(trees[256], tmp_path / 'runs', *COMMAND, '--swap-region', 'lowerbody', *extra)
        assert res.exit_code != 0 and '--swap-region needs a positive --swap_weight' in res.output, res.output
    res = _run(trees[256], tmp_path / 'runs', *COMMAND, '--swap_weight', '1', '--swap-region', 'hat')
    assert res.exit_code != 0
    # one sample per GPU round: nobody to swap with
    res = _run(trees[256], tmp_path / 'runs', *COMMAND, '--swap_weight', '1', '--gpus', '4')
    assert res.exit_code != 0 and 'at least 2 samples per GPU round' in res.output and '--batch=4 on 4 GPUs gives 1' in res.output, res.output
    res = _run(trees[256], tmp_path / 'runs', '--cfg', 'fashion', '--batch', '1', '--swap_weight', '1')
    assert res.exit_code != 0 and 'at least 2 samples per GPU round' in res.output, res.output
    assert not (tmp_path / 'runs').exists()


def test_continue_keeps_the_recorded_options_and_refuses_others(trees, tmp_path):
    from training import train_state
    import train_wo_flow_fullbody as T
    res = _run(trees[256], tmp_path / 'runs', *COMMAND, '--swap_weight', '1', '--swap-region', 'lowerbody')
    assert res.exit_code == 0, res.output
    options = _options(res.output)
    run_dir = tmp_path / 'runs' / os.path.basename(options['run_dir'])
    os.makedirs(run_dir)
    empty = dict(cur_nimg=0, batch_idx=0, cur_tick=1, elapsed_sec=0.0, num_gpus=1, batch_size=4, batch_gpu=4, random_seed=0,
                 options=json.dumps(options, indent=2), G={}, D={}, G_ema={}, opt={}, grid_z=torch.zeros([0, 0]), ranks=[])
    train_state.save_state(str(run_dir / 'training-state-000000.pt'), None, empty)
    for option, value in (('--swap_weight', '1'), ('--swap_weight', '0'), ('--swap-region', 'lowerbody'), ('--swap-region', 'fullbody')):
        res = _run(trees[256], tmp_path / 'out', '--continue', str(run_dir), option, value)
        assert res.exit_code != 0
        assert option + ' cannot be given with --continue' in res.output and 'keeps its recorded value' in res.output, res.output
    res = _run(trees[256], tmp_path / 'out', '--continue', str(run_dir))
    assert res.exit_code == 0, res.output
    got = _options(res.output)
    assert got['cfg'] == options['cfg'] and got['cfg']['loss_kwargs']['swap_weight'] == 1
    assert got['swap_outfits'] == dict(region='lowerbody', group=4)
    assert 'swap_weight' not in T.CONTINUE_MAY_CHANGE and 'swap_region' not in T.CONTINUE_MAY_CHANGE


def test_the_loss_refuses_a_negative_weight_and_missing_tensors():
    from training.loss_wo_flow_fullbody import StyleGAN2Loss
    make = lambda **kw: StyleGAN2Loss(torch.device('cpu'), None, None, None, None, None, vgg_weight=0, contextual_weight=0, **kw)
    with pytest.raises(ValueError, match='swap_weight must not be negative'):
        make(swap_weight=-1)
    assert make()._swap_inputs({}) is None and make(swap_weight=0)._swap_inputs(dict(swap_keep=1)) is None
    with pytest.raises(ValueError, match='needs the swapped tensors.*missing: swap_style_input, .*swap_keep'):
        make(swap_weight=1)._swap_inputs({})
